"""Data-parallel vocoder training: what stands between train_vocoder's GAN step and training.GradBuckets.

Each network of a trainer (`generator`, `discriminator`) gets one flat float32 device buffer, its gradient arena; every parameter's .grad is a view into
it, so the step's own backward fills the arena and GradBuckets averages slices of it over RCCL (or over gloo: two processes on one GPU, or host tensors in
the CPU tests).  The step brackets each of its two backward passes with begin(net) / finish(net); between them a hook on every parameter launches bucket
i once the last parameter of buckets 0 .. i has its gradient, so the exchange overlaps the rest of the backward.  After finish() every rank holds the same
averaged gradient, and the norm, the clip and the optimiser step run on it unchanged.

Every rank issues the same collectives in the same order whatever its data holds: buckets are launched in index order only (a bucket whose parameters
are complete waits for the ones before it), finish() launches what the hooks did not, mean_terms() averages the step's logged scalars so that the
non-finite guard takes one decision for all ranks, and same_everywhere() compares a checksum of parameters and buffers before a checkpoint is written.
"""
import os

import torch

# The largest bucket, in bytes of gradient.  A design constant, not a measurement: half of the 64 MB up to which GradBuckets issues a collective
# stream-ordered on the issuing stream (training.GradBuckets.inline_max_bytes), so that a bucket stays on that side of the limit with room to spare; the
# wire has not been timed on a multi-GPU node.
BUCKET_BYTES = 32 << 20
ALIGN = 64  # floats: 256-byte slots, as training.flat_layout; the padding stays zero
NETS = ("generator", "discriminator")


class _Arena(object):
    """one network's gradients: `flat`, the parameters in arena order with their slots, the bucket bounds (in elements) and the step's bookkeeping"""

    def __init__(self, net, bucket_bytes, group):
        from .training import GradBuckets

        self.params = [p for p in reversed(list(net.parameters())) if p.requires_grad]  # the output end finishes its backward first
        if not self.params:
            raise ValueError("fcl-taco2_amd: vocoder_dp: a network without a trainable parameter has nothing to exchange")
        for p in self.params:
            if p.dtype != torch.float32:
                raise ValueError("fcl-taco2_amd: vocoder_dp: a %s parameter; the gradient arena is float32" % p.dtype)
        sizes = [(p.numel() + ALIGN - 1) // ALIGN * ALIGN for p in self.params]
        self.offsets = [0]
        for s in sizes:
            self.offsets.append(self.offsets[-1] + s)
        # buckets are cut at parameter boundaries; a bucket is closed before the slot that would take it past bucket_bytes (one parameter larger than
        # that is a bucket of its own)
        limit, self.bounds, self.bucket_of = max(1, int(bucket_bytes) // 4), [0], []
        for j, s in enumerate(sizes):
            if self.offsets[j] > self.bounds[-1] and self.offsets[j + 1] - self.bounds[-1] > limit:
                self.bounds.append(self.offsets[j])
            self.bucket_of.append(len(self.bounds) - 1)
        self.bounds.append(self.offsets[-1])
        self.flat = torch.zeros(self.offsets[-1], dtype=torch.float32, device=self.params[0].device)
        self.views = [self.flat[o : o + p.numel()].view_as(p) for o, p in zip(self.offsets, self.params)]
        for p, v in zip(self.params, self.views):
            p.grad = v
        self.buckets = GradBuckets(self.flat, self.bounds, group)
        self.count = [self.bucket_of.count(i) for i in range(len(self.bounds) - 1)]
        self.fired, self.pending, self.next = set(), list(self.count), 0

    def launch_ready(self, everything=False):
        """launch, in index order, the buckets whose parameters all have their gradient (everything: the rest as well)"""
        while self.next < len(self.count) and (everything or self.pending[self.next] == 0):
            self.buckets.launch(self.next)
            self.next += 1


class DataParallel(object):
    """DataParallel(trainer, group=None, bucket_bytes=BUCKET_BYTES): attach to a train_vocoder.Trainer or HiFiGANTrainer (anything with .gen and .disc)
    under an initialised torch.distributed group.  FCL_VDP_OVERLAP=0 launches every bucket after backward() has returned instead of from the hooks."""

    def __init__(self, trainer, group=None, bucket_bytes=BUCKET_BYTES):
        import torch.distributed as dist

        if not (dist.is_available() and dist.is_initialized()):
            raise RuntimeError("fcl-taco2_amd: vocoder_dp: no torch.distributed process group is initialised")
        self.group, self.rank, self.world = group, dist.get_rank(group), dist.get_world_size(group)
        self.nets = {"generator": trainer.gen, "discriminator": trainer.disc}
        self.overlap = os.environ.get("FCL_VDP_OVERLAP", "1") not in ("", "0")
        self.device = next(trainer.gen.parameters()).device
        # small collectives travel on the device under RCCL and through host memory under gloo
        self.wire = self.device if dist.get_backend(group) == "nccl" else torch.device("cpu")
        for name in NETS:
            self.synchronise(name)
        self.arenas = {name: _Arena(self.nets[name], bucket_bytes, group) for name in NETS}
        self.armed, self.hooks = None, []
        for name in NETS:
            a = self.arenas[name]
            for j, p in enumerate(a.params):
                self.hooks.append(p.register_post_accumulate_grad_hook(lambda _p, a=a, j=j: self._got(a, j)))

    def detach(self):
        """remove the hooks and the views: the trainer is as before"""
        for h in self.hooks:
            h.remove()
        self.hooks = []
        for a in self.arenas.values():
            for p in a.params:
                p.grad = None

    def _got(self, a, j):
        if self.armed is not a or j in a.fired:
            return
        a.fired.add(j)
        a.pending[a.bucket_of[j]] -= 1
        if self.overlap:
            a.launch_ready()

    def begin(self, net):
        """instead of zero_grad(), which would drop the views: zero the arena, give every parameter its view again, arm the hooks of this network"""
        a = self.arenas[net]
        a.flat.zero_()
        for p, v in zip(a.params, a.views):
            if p.grad is None:
                p.grad = v
        a.fired, a.pending, a.next = set(), list(a.count), 0
        self.armed = a

    def finish(self, net):
        """launch what the hooks did not (a parameter without a gradient in this step leaves no collective unmatched), wait, and leave the averaged
        gradient in the views.  A parameter that got no gradient on this rank is handed to the optimiser as the one-GPU step hands it over, without one
        (no moment is kept for it); the networks here build the same graph on every rank, so that is the same set everywhere."""
        a = self.arenas[net]
        if self.armed is not a:
            raise RuntimeError("fcl-taco2_amd: vocoder_dp: finish(%r) without begin(%r)" % (net, net))
        self.armed = None
        a.launch_ready(everything=True)
        a.buckets.finish()
        for j, p in enumerate(a.params):
            if j not in a.fired:
                p.grad = None

    def mean_terms(self, terms):
        """the rank mean of a step's logged scalars, all of them in ONE float64 collective: every rank then sees the same values, so a non-finite term
        stops all ranks at the same step"""
        import torch.distributed as dist

        keys = list(terms)  # (the step builds them in the same order on every rank)
        t = torch.tensor([float(terms[k]) for k in keys], dtype=torch.float64, device=self.wire)
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
        return dict(zip(keys, (t / self.world).tolist()))

    def sum_float64(self, values):
        """the sum over the ranks of a list of floats (the validation sums), in float64"""
        import torch.distributed as dist

        t = torch.tensor([float(v) for v in values], dtype=torch.float64, device=self.wire)
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
        return t.tolist()

    def _state(self, net):
        m = self.nets[net]
        return list(m.named_parameters()) + list(m.named_buffers())

    def synchronise(self, net):
        """rank 0's parameters and buffers on every rank (at start-up and after load())"""
        import torch.distributed as dist

        src = dist.get_global_rank(self.group, 0) if self.group is not None else 0
        with torch.no_grad():
            for _, v in self._state(net):
                if self.wire.type == "cpu" and v.is_cuda:
                    h = v.detach().cpu()
                    dist.broadcast(h, src, group=self.group)
                    v.copy_(h)
                else:
                    dist.broadcast(v.detach(), src, group=self.group)

    def checksums(self, net):
        """-> (names, int64 [n]): per parameter and buffer, the sum of its bits read as 32-bit integers"""
        names, sums = [], []
        with torch.no_grad():
            for k, v in self._state(net):
                flat = v.detach().contiguous().view(-1)
                bits = flat.view(torch.int32) if flat.element_size() % 4 == 0 and flat.numel() else flat.to(torch.int32)
                names.append(k)
                sums.append(bits.sum(dtype=torch.int64))
        return names, torch.stack(sums)

    def same_everywhere(self, net, step):
        """raise, on every rank, unless the network's parameters and buffers (the spectral norm's power-iteration vectors among them) have the same bits
        on all ranks; called before a checkpoint of step `step` is written"""
        import torch.distributed as dist

        names, mine = self.checksums(net)
        mine = mine.to(self.wire)
        every = [torch.empty_like(mine) for _ in range(self.world)]
        dist.all_gather(every, mine, group=self.group)
        for r, other in enumerate(every):
            if not torch.equal(other, every[0]):
                bad = [names[i] for i in torch.nonzero(other != every[0]).view(-1).tolist()]
                raise RuntimeError("fcl-taco2_amd: train_vocoder: step %d: the %s of rank %d differs from rank 0's in %d tensors (%s); no checkpoint of this "
                                   "step is written" % (step, net, r, len(bad), ", ".join(bad[:5])))

    def schedule(self):
        return {net: self.arenas[net].buckets.schedule() for net in NETS}
