"""What the two Parallel WaveGAN training modules share (pwg_discriminator.py, pwg_generator.py; the device twin is csrc/pwg_rows.h): the packed batch's
row tables, the weight-norm convolution holder, and a module base with remove_weight_norm, the state-dict conversion and the plan / maps caches."""
import torch

from . import _lib

MAX_SAMPLES = 2 ** 31 - 1


class Maps(object):
    """the packed batch's rows: seg_lo / seg_hi [samples] int32 on the device, row t's utterance is [seg_lo[t], seg_hi[t])"""

    def __init__(self, lens, device):
        self.lens = [int(n) for n in lens]
        if not self.lens or min(self.lens) < 1:
            raise ValueError("fcl-taco2_amd: PWG discriminator: every utterance needs at least one sample (lens %r)" % (self.lens,))
        self.samples, self.n_utt = sum(self.lens), len(self.lens)
        if self.samples > MAX_SAMPLES:
            raise _lib.FclError("fcl-taco2_amd: more than 2^31 samples in one discriminator batch")
        ln = torch.tensor(self.lens, dtype=torch.int64)
        hi = torch.cumsum(ln, 0)
        self.seg_lo = torch.repeat_interleave(hi - ln, ln).to(torch.int32).to(device)
        self.seg_hi = torch.repeat_interleave(hi, ln).to(torch.int32).to(device)


def _norm(v):
    return torch.linalg.vector_norm(v, dim=tuple(range(1, v.dim())), keepdim=True)


class _Conv(torch.nn.Module):
    """the parameters of one convolution under the reference's names: weight (and bias), or weight_g / weight_v under weight norm"""

    def __init__(self, shape, bias, weight_norm, init=None):
        super().__init__()
        w = torch.empty(*shape)
        if init is None:
            torch.nn.init.kaiming_normal_(w, nonlinearity="relu")
        else:
            w.fill_(init)
        if weight_norm:
            self.weight_g = torch.nn.Parameter(_norm(w))
            self.weight_v = torch.nn.Parameter(w)
        else:
            self.weight = torch.nn.Parameter(w)
        self.register_parameter("bias", torch.nn.Parameter(torch.zeros(shape[0])) if bias else None)

    def folded(self):
        """w = v g / ||v|| over every dim but 0 (torch.nn.utils.weight_norm with dim 0), in torch operations so that autograd carries it"""
        if "weight" in self._parameters:
            return self.weight
        return self.weight_v * (self.weight_g / _norm(self.weight_v))


class _Module(torch.nn.Module):
    """a module of _Conv holders; a subclass sets CHECKPOINT_KEY (its entry of a parallel_wavegan checkpoint's "model") and PLAN (its plan class, built
    from the device and self.config) and calls _reset_cache() in __init__"""

    def _reset_cache(self):
        self._plan, self._maps_key, self._maps = None, None, None

    def _named_convs(self):
        """[(state-dict prefix, _Conv)]"""
        return [(name + ".", m) for name, m in self.named_modules() if isinstance(m, _Conv)]

    def remove_weight_norm(self):
        """fold weight_g / weight_v into weight"""
        for _, m in self._named_convs():
            if "weight" not in m._parameters:
                w = m.folded().detach()
                del m.weight_g, m.weight_v
                m.weight = torch.nn.Parameter(w)
        self.use_weight_norm = False

    def load_state_dict(self, state_dict, strict=True):
        """either form of the names (a weight-norm dict into a plain module is folded, a plain one into a weight-norm module gets g = ||w||), or a
        whole parallel_wavegan checkpoint ({"model": {CHECKPOINT_KEY: ...}})"""
        sd = state_dict
        if "model" in sd and isinstance(sd["model"], dict) and self.CHECKPOINT_KEY in sd["model"]:
            sd = sd["model"][self.CHECKPOINT_KEY]
        sd = {k: torch.as_tensor(v) for k, v in sd.items()}
        for p, m in self._named_convs():
            plain = "weight" in m._parameters
            if plain and p + "weight_v" in sd:
                v, g = sd.pop(p + "weight_v"), sd.pop(p + "weight_g")
                sd[p + "weight"] = v * (g / _norm(v))
            elif not plain and p + "weight" in sd:
                w = sd.pop(p + "weight")
                sd[p + "weight_v"], sd[p + "weight_g"] = w, _norm(w)
        return super().load_state_dict(sd, strict=strict)

    def plan(self):
        dev = next(self.parameters()).device
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda:%d" % torch.cuda.current_device())
        if self._plan is None or self._plan.device != dev:
            self._plan = self.PLAN(dev, **self.config)
            self._maps_key = None
        return self._plan

    def maps(self, lens):
        """kept for the next batch of the same lengths"""
        key = tuple(lens)
        if key != self._maps_key:
            self._maps_key, self._maps = key, Maps(lens, self.plan().device)
        return self._maps
