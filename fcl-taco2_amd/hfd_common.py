"""What the two HiFi-GAN discriminator modules share (hifigan_discriminator.py, hifigan_scale_discriminator.py; the device twin is csrc/hfd_rows.h; DESIGN.md
§6t): the table-driven row geometry of a stack of strided convolutions, the plan base with the sizes of a pass, the launches of a forward and a backward
pass on caller-owned buffers, the autograd function over them, the input forms and the module base.

A plan's geometry is one (cin, cout, taps, stride, pad) or (cin, cout, taps, stride, pad, groups) per layer, the score layer last.  The launches ask the
plan which entries run a layer (`plan.hsd(layer)`: the fcl_hsd_* ones with fcl_hsd_t, else the fcl_hpd_* ones with fcl_hpd_t) and whether the module's
weights are Conv2d-shaped (`plan.CONV2D`: a trailing kernel axis of 1)."""
import ctypes as C

import numpy as np
import torch

from . import _lib, ops
from .pwg_common import _Module

_PACK_WHO = "fcl-taco2_amd: HiFi-GAN period discriminator"  # (pack_input began in the period module and both kinds of module report under its name)


def out_rows(h, taps, stride, pad):
    return (h + 2 * pad - taps) // stride + 1


def segment_tables(h_in, k, s, pad, device):
    """segments of h_in rows back to back under one layer -> the int32 device tables (src, in_lo, in_hi) at the rate of its output rows"""
    h_in = np.asarray(h_in, dtype=np.int64)
    h_out = out_rows(h_in, k, s, pad)
    lo = np.repeat(np.cumsum(h_in) - h_in, h_out)
    o = np.arange(h_out.sum()) - np.repeat(np.cumsum(h_out) - h_out, h_out)
    tab = lambda a: torch.from_numpy(a.astype(np.int32)).to(device)
    return tab(lo + s * o), tab(lo), tab(lo + np.repeat(h_in, h_out))


class LayerMaps(object):
    """the tables of one layer alone over segments of the given heights (what PeriodMaps / ScaleMaps hold per layer), for launches on given inputs"""

    def __init__(self, h_in, k, s, pad, device):
        self.rows = [int(np.sum(h_in)), int(np.sum(out_rows(np.asarray(h_in, dtype=np.int64), k, s, pad)))]
        src, lo, hi = segment_tables(h_in, k, s, pad, device)
        self.src, self.in_lo, self.in_hi = [src], [lo], [hi]


def activation_slope(who, nonlinear_activation_params, negative_slope):
    """the LeakyReLU slope of a constructor's nonlinear_activation_params / negative_slope pair; any other activation parameter is refused"""
    params = dict(nonlinear_activation_params or {"negative_slope": 0.1})
    if negative_slope is not None:
        params["negative_slope"] = negative_slope
    extra = sorted(set(params) - {"negative_slope", "inplace"})
    if extra:
        raise ValueError("%s: nonlinear_activation_params=%r is not supported on the HIP path (negative_slope only)" % (who, extra))
    return params.get("negative_slope", 0.01)


class Plan(object):
    """Per-layer geometry, the score layer last, and the sizes of what a pass needs.  A subclass sets geometry, period (segments per utterance), slope and
    bias, calls _on(device), and may override hsd()."""

    CONV2D = False

    def _on(self, device):
        self.layers = len(self.geometry)  # the score layer included
        if not str(device).startswith("cuda"):
            raise _lib.FclError("fcl-taco2_amd: %s needs a GPU device (no CPU fallback)" % type(self).__name__)
        self.device, self._slot_index = torch.device(device), {}

    def hsd(self, layer):
        """whether the fcl_hsd_* entries run this layer"""
        return False

    def groups(self, layer):
        g = self.geometry[layer]
        return g[5] if len(g) > 5 else 1

    def heights(self, n):
        """rows of one segment of an utterance of n samples: [H0, H1, .., H_last, H_score]"""
        hs = [-(-int(n) // self.period)]
        for g in self.geometry:
            hs.append(out_rows(hs[-1], g[2], g[3], g[4]))
        return hs

    def rows(self, lens):
        """rows per level of a batch: rows[0] the (padded) waveform's samples, rows[l + 1] the output rows of layer l"""
        per = [self.heights(int(n)) for n in lens]
        return [self.period * sum(h[l] for h in per) for l in range(self.layers + 1)]

    def act_shapes(self, rows):
        """the outputs of a pass: map_0 .. map_{L-1} [rows[l + 1], cout_l] and the scores [rows[L + 1]]"""
        return [(rows[l + 1], g[1]) for l, g in enumerate(self.geometry[:-1])] + [(rows[-1],)]

    def kept_bytes(self, lens):
        """what a forward pass keeps for the backward pass: the packed waveform and every map"""
        rows = self.rows(lens)
        return 4 * (rows[0] + sum(n * c for n, c in self.act_shapes(rows)[:-1]))

    def workspace_floats(self, rows):
        """the partials of the largest layer's weight gradient"""
        lib, need = _lib.load(), 0
        for l, g in enumerate(self.geometry):
            if self.hsd(l):
                need = max(need, lib.fcl_hsd_dw_workspace_bytes(rows[l + 1], g[0], g[1], self.groups(l), g[2]))
            else:
                need = max(need, lib.fcl_hpd_dw_workspace_bytes(rows[l + 1], g[0], g[1], g[2]))
        return need // 4

    def dweight_shapes(self):
        """per layer (dw [taps, cin / groups, cout], db [cout]) in the kernels' tap-major layout"""
        return [((g[2], g[0] // self.groups(l), g[1]), (g[1],)) for l, g in enumerate(self.geometry)]

    def slot_index(self, layer):
        """which tap (taps: none) each slot of the per-phase input-gradient weights holds, [stride x ceil(taps / stride)] int64 on the device"""
        if layer not in self._slot_index:
            k, s, pad = self.geometry[layer][2:5]
            slots = -(-k // s)
            idx = [[(ph + pad) % s + s * i for i in range(slots)] for ph in range(s)]
            self._slot_index[layer] = torch.tensor([j if j < k else k for row in idx for j in row], dtype=torch.int64, device=self.device)
        return self._slot_index[layer]


def pack_weights(plan, weights, biases, backward=True):
    """torch weights [cout, cin / groups, taps] (Conv2d-shaped under plan.CONV2D: a trailing 1) -> per layer (wf [taps, cin / groups, cout], wb, bias or
    None), contiguous; wb is the input gradient's operand: for a C -> C' layer [stride, ceil(taps / stride), cout / groups, cin] (slot i of phase ph holds
    tap (ph + pad) % stride + stride i of the column's own group, or zeros), else wf itself"""
    out = []
    for l, (w, b) in enumerate(zip(weights, biases)):
        w = w.detach().to(torch.float32)
        if plan.CONV2D:
            w = w[..., 0]
        wf, wb = w.permute(2, 1, 0).contiguous(), None
        if backward:
            ci, co, k = plan.geometry[l][:3]
            if ci > 1 and co > 1:
                gr = plan.groups(l)
                cog, cig = co // gr, ci // gr
                taps = w.reshape(gr, cog, cig, k).permute(3, 1, 0, 2).reshape(k, cog, ci)
                taps = torch.cat([taps, w.new_zeros(1, cog, ci)])
                wb = taps.index_select(0, plan.slot_index(l)).contiguous()
            else:
                wb = wf
        out.append((wf, wb, None if b is None else b.detach().to(torch.float32).contiguous()))
    return out


def unpack_dweights(dws, conv2d=False):
    """the kernels' [taps, cin / groups, cout] -> torch's [cout, cin / groups, taps] (conv2d: [cout, cin, taps, 1])"""
    return [(dw.permute(2, 1, 0).unsqueeze(-1) if conv2d else dw.permute(2, 1, 0)).contiguous() for dw in dws]


def _args(plan, maps, layer, **ptr):
    ci, co, k, s, pad = plan.geometry[layer][:5]
    hsd = plan.hsd(layer)
    a = _lib.HsdLayer() if hsd else _lib.HpdLayer()
    a.rows_in, a.rows_out, a.cin, a.cout, a.ksize, a.stride, a.pad, a.slope = maps.rows[layer], maps.rows[layer + 1], ci, co, k, s, pad, plan.slope
    if hsd:
        a.groups = plan.groups(layer)
    a.src, a.in_lo, a.in_hi = maps.src[layer].data_ptr(), maps.in_lo[layer].data_ptr(), maps.in_hi[layer].data_ptr()
    for key, v in ptr.items():
        if v is not None:
            setattr(a, key, v.data_ptr())
    return a


def _entry(plan, layer, what):
    return getattr(_lib.load(), ("fcl_hsd_layer_" if plan.hsd(layer) else "fcl_hpd_layer_") + what)


# on caller-owned buffers (the tests surround them with guard zones)
def launch_forward(plan, maps, x, weights, acts):
    """x [rows[0]] float32 (the packed waveform; phase-major and padded under a period), weights from pack_weights -> acts: the maps and the scores
    (plan.act_shapes)"""
    st = ops._stream()
    src = x
    for l, (wf, _, b) in enumerate(weights):
        _lib.check(_entry(plan, l, "fwd")(C.byref(_args(plan, maps, l, x=src, w=wf, bias=b, y=acts[l])), st))
        src = acts[l]


def launch_backward(plan, maps, dscore, extras, weights, acts, gx, dweights, x=None, grads=None, workspace=None):
    """dscore [rows[L + 1]], extras: per map its direct gradient [rows, C] or None -> gx [rows[0]] (None: the waveform gradient is not computed) and dweights =
    [(dw [taps, cin / groups, cout], db [cout] or None)] per layer (None: no weight gradient is computed).  acts: the maps; x: the packed waveform (needed
    with dweights); grads: one buffer per map, of its size; workspace: plan.workspace_floats(rows) floats (needed with dweights)."""
    st = ops._stream()
    g = dscore
    for l in range(plan.layers - 1, -1, -1):
        _, wb, _ = weights[l]
        below = x if l == 0 else acts[l - 1]
        if dweights is not None:
            dw, db = dweights[l]
            a = _args(plan, maps, l, x=below, g=g, dw=dw, db=db, workspace=workspace)
            a.workspace_bytes = workspace.numel() * 4
            _lib.check(_entry(plan, l, "dw")(C.byref(a), st))
        if l > 0:
            _lib.check(_entry(plan, l, "dx")(C.byref(_args(plan, maps, l, g=g, w=wb, h=below, extra=extras[l - 1], y=grads[l - 1])), st))
            g = grads[l - 1]
        elif gx is not None:
            _lib.check(_entry(plan, l, "dx")(C.byref(_args(plan, maps, l, g=g, w=wb, y=gx)), st))


class _Function(torch.autograd.Function):
    """every map and the scores of the packed waveform under plain weights and biases; backward takes a gradient for each output (None: none) and gives
    the gradients of all inputs that are asked for"""

    @staticmethod
    def forward(ctx, plan, maps, x, *params):
        L, dev = plan.layers, plan.device
        ws, bs = params[:L], params[L:] if plan.bias else [None] * L
        with torch.cuda.device(dev):
            x = x.detach().contiguous()
            packed = pack_weights(plan, ws, bs, backward=any(ctx.needs_input_grad))
            acts = [torch.empty(s, device=dev, dtype=torch.float32) for s in plan.act_shapes(maps.rows)]
            launch_forward(plan, maps, x, packed, acts)
        ctx.plan, ctx.maps, ctx.packed = plan, maps, packed
        ctx.save_for_backward(x, *acts[:-1])
        ctx.set_materialize_grads(False)
        return tuple(acts)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *douts):
        plan, maps, dev = ctx.plan, ctx.maps, ctx.plan.device
        x, acts = ctx.saved_tensors[0], list(ctx.saved_tensors[1:])
        need_x, need_w = ctx.needs_input_grad[2], any(ctx.needs_input_grad[3:])
        with torch.cuda.device(dev):
            new = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
            f32 = lambda g: None if g is None else g.detach().to(torch.float32).contiguous()
            dscore = f32(douts[-1]) if douts[-1] is not None else torch.zeros(maps.rows[-1], device=dev, dtype=torch.float32)
            gx = new(maps.rows[0]) if need_x else None
            dweights = [(new(sw), new(sb) if plan.bias else None) for sw, sb in plan.dweight_shapes()] if need_w else None
            launch_backward(plan, maps, dscore, [f32(g) for g in douts[:-1]], ctx.packed, acts, gx, dweights, x=x,
                            grads=[new(a.shape) for a in acts], workspace=new(plan.workspace_floats(maps.rows)) if need_w else None)
        out = [None, None, gx]
        if need_w:
            out += unpack_dweights([dw for dw, _ in dweights], plan.CONV2D) + ([db for _, db in dweights] if plan.bias else [])
        else:
            out += [None] * (len(ctx.needs_input_grad) - 3)
        return tuple(out)


class _Activation(torch.nn.Module):  # index 1 of each entry of a module's layer list, as the package's Sequential of convolution and activation
    pass


def pack_input(x, lens, device):
    """[B, T], [B, 1, T] or packed 1-D with lens -> (packed x, lens); torch operations, so the padding of a [B, T] input with lens gets zero gradient"""
    x = torch.as_tensor(x)
    if x.dim() == 3:
        if x.shape[1] != 1:
            raise ValueError("%s: a 3-D input must be [B, 1, T], got %r" % (_PACK_WHO, tuple(x.shape)))
        x = x[:, 0]
    x = x.to(device=device, dtype=torch.float32)
    if x.dim() == 1:
        lens = [int(x.numel())] if lens is None else [int(n) for n in lens]
        if sum(lens) != x.numel():
            raise ValueError("%s: the packed waveform has %d samples, lens sum to %d" % (_PACK_WHO, x.numel(), sum(lens)))
        return x.contiguous(), lens
    if x.dim() != 2:
        raise ValueError("%s: [B, T], [B, 1, T] or packed 1-D input expected, got %r" % (_PACK_WHO, tuple(x.shape)))
    B, T = x.shape
    if lens is None:
        return x.reshape(-1).contiguous(), [int(T)] * int(B)
    lens = [int(n) for n in lens]
    if len(lens) != B or max(lens) > T or min(lens) < 1:
        raise ValueError("%s: lens %r do not fit an input of %r" % (_PACK_WHO, lens, tuple(x.shape)))
    return torch.cat([x[b, :n] for b, n in enumerate(lens)]).contiguous(), lens


class _Discriminator(_Module):
    """one stack of convolutions: a subclass sets PLAN, MAPS (the row tables of a batch under the plan) and conv_list() (the holders, the score layer last)"""

    CHECKPOINT_KEY = "discriminator"

    def maps(self, lens):
        """kept for the next batch of the same lengths"""
        key = tuple(lens)
        plan = self.plan()
        if key != self._maps_key:
            self._maps_key, self._maps = key, self.MAPS(plan, lens)
        return self._maps

    def forward_packed(self, x, lens):
        plan, maps = self.plan(), self.maps(lens)
        convs = self.conv_list()
        params = [m.folded() for m in convs] + ([m.bias for m in convs] if self.config["bias"] else [])
        gather = getattr(maps, "gather", None)  # (a period's phase-major, reflection-padded order)
        return list(_Function.apply(plan, maps, x if gather is None else x.index_select(0, gather), *params))

    def forward(self, x, lens=None):
        x, lens = pack_input(x, lens, self.plan().device)
        return self.forward_packed(x, lens)
