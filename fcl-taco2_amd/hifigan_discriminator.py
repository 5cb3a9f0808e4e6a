"""The HiFi-GAN multi-period discriminator on the HIP path, with its backward pass (the hpd_* kernels of csrc/hifigan_disc.hip).

One period discriminator folds the waveform by its period p -- [B, 1, T] is reflection-padded on the right to a multiple of p and viewed as [B, 1, H0, p] --
and runs Conv2d(cin -> cout, (k0, 1), stride (s, 1), padding ((k0 - 1) / 2, 0)) + LeakyReLU per downsample scale (widths channels, x 4 per layer up to
max_downsample_channels), then output_conv = Conv2d(C -> 1, (k1 - 1, 1), padding ((k1 - 1) / 2, 0)) without activation.  It returns every layer's
post-activation map and, last, the scores.  The multi-period discriminator holds one of them per period.  The published architecture (Kong et al. 2020)
as parallel_wavegan's HiFiGANPeriodDiscriminator / HiFiGANMultiPeriodDiscriminator states it; parity with the package's checkpoints is by parameter names
and shapes, not pinned against its code.

    mpd = HiFiGANMultiPeriodDiscriminator().to("cuda:0")
    outs = mpd(wave)                     # [B, T], [B, 1, T] or packed 1-D with lens= -> per period [map_0 .. map_{L-1}, scores], packed
    generator_adversarial_loss(outs).backward()

The contract is stated in include/fcl_hip.h "HiFi-GAN period discriminator" and restated in float64 numpy in tests/hfgd_ref.py.  Activations are float32,
channel-last [rows, C]; for period p an utterance is p segments (one per phase), phase-major, the segments back to back, so the outputs are packed:
[rows_l, C_l] maps and [rows_score] scores (to_reference_layout gives the package's views for equal lengths).  Only the post-activations are kept for
the backward pass.  One arithmetic mode (exact fp32).  No CPU fallback."""
import ctypes as C

import numpy as np
import torch

from . import _lib, ops
from .pwg_common import MAX_SAMPLES, _Conv, _Module

KERNEL_SIZES_0, KERNEL_SIZES_1 = (3, 5), (3, 4)
PERIODS = (2, 3, 5, 7, 11)
WHO = "fcl-taco2_amd: HiFi-GAN period discriminator"


def check_lengths(period, lens):
    """an utterance must be long enough to be reflection-padded to a multiple of the period"""
    lens = [int(n) for n in lens]
    for n in lens:
        if n < 1 or (n % period and period - n % period >= n):
            raise ValueError("%s: lens=%r: an utterance of %d samples cannot be reflection-padded to a multiple of period %d" % (WHO, lens, n, period))
    return lens


def check_configuration(in_channels=1, out_channels=1, period=3, kernel_sizes=(5, 3), channels=32, downsample_scales=(3, 3, 3, 3, 1),
                        max_downsample_channels=1024, bias=True, nonlinear_activation="LeakyReLU", negative_slope=0.1, use_weight_norm=True,
                        use_spectral_norm=False, lens=None):
    """-> [(cin, cout, taps, stride, pad)] per layer, the score layer last; anything the kernels do not cover is refused by the argument's name"""
    bad = lambda name, got, want: ValueError("%s: %s=%r is not supported on the HIP path (%s)" % (WHO, name, got, want))
    width = lambda c: isinstance(c, int) and 16 <= c <= 1024 and c % 16 == 0
    if in_channels != 1:
        raise bad("in_channels", in_channels, "1")
    if out_channels != 1:
        raise bad("out_channels", out_channels, "1")
    if not (isinstance(period, int) and 1 <= period <= 16):
        raise bad("period", period, "1 to 16")
    ks = tuple(kernel_sizes) if isinstance(kernel_sizes, (tuple, list)) else ()
    if len(ks) != 2 or ks[0] not in KERNEL_SIZES_0 or ks[1] not in KERNEL_SIZES_1:
        raise bad("kernel_sizes", kernel_sizes, "(3 or 5, 3 or 4)")
    if not width(channels):
        raise bad("channels", channels, "a multiple of 16 from 16 to 1024")
    if not width(max_downsample_channels):
        raise bad("max_downsample_channels", max_downsample_channels, "a multiple of 16 from 16 to 1024")
    sc = tuple(downsample_scales) if isinstance(downsample_scales, (tuple, list)) else ()
    if not (1 <= len(sc) <= 8 and all(isinstance(s, int) and 1 <= s <= 4 for s in sc)):
        raise bad("downsample_scales", downsample_scales, "1 to 8 scales from 1 to 4")
    if bias not in (True, False):
        raise bad("bias", bias, "True or False")
    if nonlinear_activation != "LeakyReLU":
        raise bad("nonlinear_activation", nonlinear_activation, "LeakyReLU")
    if not 0.0 <= float(negative_slope) < 1.0:
        raise bad("negative_slope", negative_slope, "0 <= negative_slope < 1")
    if use_weight_norm not in (True, False):
        raise bad("use_weight_norm", use_weight_norm, "True or False")
    if use_spectral_norm:
        raise bad("use_spectral_norm", use_spectral_norm, "False")
    if lens is not None:
        check_lengths(period, lens)
    geo, ci, co = [], 1, channels
    for s in sc:
        geo.append((ci, co, ks[0], s, (ks[0] - 1) // 2))
        ci, co = co, min(4 * co, max_downsample_channels)
    geo.append((ci, 1, ks[1] - 1, 1, (ks[1] - 1) // 2))
    return geo


def out_rows(h, taps, stride, pad):
    return (h + 2 * pad - taps) // stride + 1


class PeriodPlan(object):
    """Per-layer geometry (cin, cout, taps, stride, pad), the score layer last, and the sizes of what a pass needs"""

    def __init__(self, device="cuda:0", **config):
        config = {k: v for k, v in config.items() if k != "lens"}
        self.geometry = check_configuration(**config)
        cfg = dict(period=3, negative_slope=0.1, bias=True)
        cfg.update({k: v for k, v in config.items() if k in cfg})
        self.period, self.slope, self.bias = cfg["period"], float(cfg["negative_slope"]), bool(cfg["bias"])
        self.layers = len(self.geometry)  # the score layer included
        if not str(device).startswith("cuda"):
            raise _lib.FclError("fcl-taco2_amd: PeriodPlan needs a GPU device (no CPU fallback)")
        self.device = torch.device(device)
        self._slot_index = {}

    def heights(self, n):
        """rows of one segment of an utterance of n samples: [H0, H1, .., H_last, H_score]"""
        hs = [-(-n // self.period)]
        for _, _, k, s, pad in self.geometry:
            hs.append(out_rows(hs[-1], k, s, pad))
        return hs

    def rows(self, lens):
        """rows per level of a batch: rows[0] the padded waveform's samples, rows[l + 1] the output rows of layer l"""
        per = [self.heights(int(n)) for n in lens]
        return [self.period * sum(h[l] for h in per) for l in range(self.layers + 1)]

    def act_shapes(self, rows):
        """the outputs of a pass: map_0 .. map_{L-1} [rows[l + 1], cout_l] and the scores [rows[L + 1]]"""
        return [(rows[l + 1], co) for l, (_, co, _, _, _) in enumerate(self.geometry[:-1])] + [(rows[-1],)]

    def kept_bytes(self, lens):
        """what a forward pass keeps for the backward pass: the packed waveform and every map"""
        rows = self.rows(lens)
        return 4 * (rows[0] + sum(n * c for n, c in self.act_shapes(rows)[:-1]))

    def workspace_floats(self, rows):
        """the partials of the largest layer's weight gradient"""
        lib = _lib.load()
        return max(lib.fcl_hpd_dw_workspace_bytes(rows[l + 1], ci, co, k) for l, (ci, co, k, _, _) in enumerate(self.geometry)) // 4

    def dweight_shapes(self):
        """per layer (dw [taps, cin, cout], db [cout]) in the kernels' tap-major layout"""
        return [((k, ci, co), (co,)) for ci, co, k, _, _ in self.geometry]

    def slot_index(self, layer):
        """which tap (taps: none) each slot of the per-phase input-gradient weights holds, [stride x ceil(taps / stride)] int64 on the device"""
        if layer not in self._slot_index:
            _, _, k, s, pad = self.geometry[layer]
            slots = -(-k // s)
            idx = [[(ph + pad) % s + s * i for i in range(slots)] for ph in range(s)]
            self._slot_index[layer] = torch.tensor([j if j < k else k for row in idx for j in row], dtype=torch.int64, device=self.device)
        return self._slot_index[layer]


class LayerPlan(PeriodPlan):
    """one layer alone (what PeriodPlan holds per layer), for launches on given inputs"""

    def __init__(self, device, cin, cout, taps, stride, pad, slope=0.1):
        self.geometry, self.period, self.slope, self.bias, self.layers = [(cin, cout, taps, stride, pad)], 1, float(slope), True, 1
        self.device, self._slot_index = torch.device(device), {}


class PeriodMaps(object):
    """the rows of a packed batch under one period: per layer l the int32 device tables src / in_lo / in_hi at the rate of its output rows, the row counts
    per level, and `gather` [rows[0]] int64, which picks the phase-major, reflection-padded waveform out of the packed one"""

    def __init__(self, plan, lens):
        p = plan.period
        self.lens = check_lengths(p, lens)
        if not self.lens:
            raise ValueError("%s: lens=%r: an empty batch" % (WHO, self.lens))
        self.samples, self.n_utt = sum(self.lens), len(self.lens)
        per = np.array([plan.heights(n) for n in self.lens], dtype=np.int64)  # [utt, level]
        self.rows = [int(p * per[:, l].sum()) for l in range(plan.layers + 1)]
        if max(self.rows) > MAX_SAMPLES or self.samples > MAX_SAMPLES:
            raise _lib.FclError("fcl-taco2_amd: more than 2^31 rows in one period-discriminator batch")
        dev = plan.device
        ln = np.array(self.lens, dtype=np.int64)
        off = np.cumsum(ln) - ln
        # the waveform: segment (b, q) holds x_pad[b, h p + q], h = 0 .. H0 - 1; x_pad[T + i] = x[T - 2 - i]
        seg_h = np.repeat(per[:, 0], p)
        seg_u = np.repeat(np.arange(self.n_utt), p)
        seg_q = np.tile(np.arange(p), self.n_utt)
        row_seg = np.repeat(np.arange(seg_h.size), seg_h)
        h = np.arange(seg_h.sum()) - np.repeat(np.cumsum(seg_h) - seg_h, seg_h)
        n = h * p + seg_q[row_seg]
        T = ln[seg_u[row_seg]]
        self.gather = torch.from_numpy(off[seg_u[row_seg]] + np.where(n < T, n, 2 * (T - 1) - n)).to(dev)
        self.src, self.in_lo, self.in_hi = [], [], []
        for l, (_, _, k, s, pad) in enumerate(plan.geometry):
            src, lo, hi = segment_tables(np.repeat(per[:, l], p), k, s, pad, dev)
            self.src.append(src), self.in_lo.append(lo), self.in_hi.append(hi)


def segment_tables(h_in, k, s, pad, device):
    """segments of h_in rows back to back under one layer -> the int32 device tables (src, in_lo, in_hi) at the rate of its output rows"""
    h_in = np.asarray(h_in, dtype=np.int64)
    h_out = out_rows(h_in, k, s, pad)
    lo = np.repeat(np.cumsum(h_in) - h_in, h_out)
    o = np.arange(h_out.sum()) - np.repeat(np.cumsum(h_out) - h_out, h_out)
    tab = lambda a: torch.from_numpy(a.astype(np.int32)).to(device)
    return tab(lo + s * o), tab(lo), tab(lo + np.repeat(h_in, h_out))


class LayerMaps(object):
    """the tables of one layer alone over segments of the given heights (what PeriodMaps holds per layer), for launches on given inputs"""

    def __init__(self, h_in, k, s, pad, device):
        self.rows = [int(np.sum(h_in)), int(np.sum(out_rows(np.asarray(h_in, dtype=np.int64), k, s, pad)))]
        src, lo, hi = segment_tables(h_in, k, s, pad, device)
        self.src, self.in_lo, self.in_hi = [src], [lo], [hi]


def pack_weights(plan, weights, biases, backward=True):
    """torch Conv2d weights [cout, cin, taps, 1] -> per layer (wf [taps, cin, cout], wb, bias or None), contiguous; wb is the input gradient's operand: for a
    C -> C' layer [stride, ceil(taps / stride), cout, cin] (slot i of phase ph holds tap (ph + pad) % stride + stride i, or zeros), else wf itself"""
    out = []
    for l, (w, b) in enumerate(zip(weights, biases)):
        w = w.detach().to(torch.float32)[..., 0]
        wf, wb = w.permute(2, 1, 0).contiguous(), None
        if backward:
            ci, co, k, s, _ = plan.geometry[l]
            if ci > 1 and co > 1:
                taps = torch.cat([w.permute(2, 0, 1), w.new_zeros(1, co, ci)])
                wb = taps.index_select(0, plan.slot_index(l)).contiguous()
            else:
                wb = wf
        out.append((wf, wb, None if b is None else b.detach().to(torch.float32).contiguous()))
    return out


def unpack_dweights(dws):
    """the kernels' [taps, cin, cout] -> torch's [cout, cin, taps, 1]"""
    return [dw.permute(2, 1, 0).unsqueeze(-1).contiguous() for dw in dws]


def _args(plan, maps, layer, **ptr):
    ci, co, k, s, pad = plan.geometry[layer]
    a = _lib.HpdLayer()
    a.rows_in, a.rows_out, a.cin, a.cout, a.ksize, a.stride, a.pad, a.slope = maps.rows[layer], maps.rows[layer + 1], ci, co, k, s, pad, plan.slope
    a.src, a.in_lo, a.in_hi = maps.src[layer].data_ptr(), maps.in_lo[layer].data_ptr(), maps.in_hi[layer].data_ptr()
    for key, v in ptr.items():
        if v is not None:
            setattr(a, key, v.data_ptr())
    return a


# on caller-owned buffers (the tests surround them with guard zones)
def launch_forward(plan, maps, x, weights, acts):
    """x [rows[0]] float32 (the phase-major padded waveform), weights from pack_weights -> acts: the maps and the scores (plan.act_shapes)"""
    lib, st = _lib.load(), ops._stream()
    src = x
    for l, (wf, _, b) in enumerate(weights):
        _lib.check(lib.fcl_hpd_layer_fwd(C.byref(_args(plan, maps, l, x=src, w=wf, bias=b, y=acts[l])), st))
        src = acts[l]


def launch_backward(plan, maps, dscore, extras, weights, acts, gx, dweights, x=None, grads=None, workspace=None):
    """dscore [rows[L + 1]], extras: per map its direct gradient [rows, C] or None -> gx [rows[0]] (None: the waveform gradient is not computed) and dweights =
    [(dw [taps, cin, cout], db [cout] or None)] per layer (None: no weight gradient is computed).  acts: the maps; x: the packed waveform (needed with
    dweights); grads: one buffer per map, of its size; workspace: plan.workspace_floats(rows) floats (needed with dweights)."""
    lib, st = _lib.load(), ops._stream()
    g = dscore
    for l in range(plan.layers - 1, -1, -1):
        _, wb, _ = weights[l]
        below = x if l == 0 else acts[l - 1]
        if dweights is not None:
            dw, db = dweights[l]
            a = _args(plan, maps, l, x=below, g=g, dw=dw, db=db, workspace=workspace)
            a.workspace_bytes = workspace.numel() * 4
            _lib.check(lib.fcl_hpd_layer_dw(C.byref(a), st))
        if l > 0:
            _lib.check(lib.fcl_hpd_layer_dx(C.byref(_args(plan, maps, l, g=g, w=wb, h=below, extra=extras[l - 1], y=grads[l - 1])), st))
            g = grads[l - 1]
        elif gx is not None:
            _lib.check(lib.fcl_hpd_layer_dx(C.byref(_args(plan, maps, l, g=g, w=wb, y=gx)), st))


class _Function(torch.autograd.Function):
    """every map and the scores of the phase-major packed waveform under plain weights and biases; backward takes a gradient for each output (None: none)
    and gives the gradients of all inputs that are asked for"""

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
            out += unpack_dweights([dw for dw, _ in dweights]) + ([db for _, db in dweights] if plan.bias else [])
        else:
            out += [None] * (len(ctx.needs_input_grad) - 3)
        return tuple(out)


class _Activation(torch.nn.Module):  # index 1 of each entry of convs, as the package's Sequential of convolution and activation
    pass


def pack_input(x, lens, device):
    """[B, T], [B, 1, T] or packed 1-D with lens -> (packed x, lens); torch operations, so the padding of a [B, T] input with lens gets zero gradient"""
    x = torch.as_tensor(x)
    if x.dim() == 3:
        if x.shape[1] != 1:
            raise ValueError("%s: a 3-D input must be [B, 1, T], got %r" % (WHO, tuple(x.shape)))
        x = x[:, 0]
    x = x.to(device=device, dtype=torch.float32)
    if x.dim() == 1:
        lens = [int(x.numel())] if lens is None else [int(n) for n in lens]
        if sum(lens) != x.numel():
            raise ValueError("%s: the packed waveform has %d samples, lens sum to %d" % (WHO, x.numel(), sum(lens)))
        return x.contiguous(), lens
    if x.dim() != 2:
        raise ValueError("%s: [B, T], [B, 1, T] or packed 1-D input expected, got %r" % (WHO, tuple(x.shape)))
    B, T = x.shape
    if lens is None:
        return x.reshape(-1).contiguous(), [int(T)] * int(B)
    lens = [int(n) for n in lens]
    if len(lens) != B or max(lens) > T or min(lens) < 1:
        raise ValueError("%s: lens %r do not fit an input of %r" % (WHO, lens, tuple(x.shape)))
    return torch.cat([x[b, :n] for b, n in enumerate(lens)]).contiguous(), lens


class HiFiGANPeriodDiscriminator(_Module):
    """forward(x, lens=None) -> [map_0, .., map_{L-1}, scores], packed.  Parameters: convs.{l}.0.weight / .bias and output_conv.weight / .bias (weight_g /
    weight_v under use_weight_norm), Conv2d-shaped [cout, cin, k, 1]; Kaiming-normal weights, zero biases."""

    CHECKPOINT_KEY, PLAN = "discriminator", PeriodPlan

    def __init__(self, in_channels=1, out_channels=1, period=3, kernel_sizes=(5, 3), channels=32, downsample_scales=(3, 3, 3, 3, 1),
                 max_downsample_channels=1024, bias=True, nonlinear_activation="LeakyReLU", nonlinear_activation_params=None, use_weight_norm=True,
                 use_spectral_norm=False, negative_slope=None):
        super().__init__()
        params = dict(nonlinear_activation_params or {"negative_slope": 0.1})
        if negative_slope is not None:
            params["negative_slope"] = negative_slope
        extra = sorted(set(params) - {"negative_slope", "inplace"})
        if extra:
            raise ValueError("%s: nonlinear_activation_params=%r is not supported on the HIP path (negative_slope only)" % (WHO, extra))
        self.config = dict(in_channels=in_channels, out_channels=out_channels, period=period, kernel_sizes=tuple(kernel_sizes), channels=channels,
                           downsample_scales=tuple(downsample_scales), max_downsample_channels=max_downsample_channels, bias=bias,
                           nonlinear_activation=nonlinear_activation, negative_slope=params.get("negative_slope", 0.01),
                           use_weight_norm=use_weight_norm, use_spectral_norm=use_spectral_norm)
        geo = check_configuration(**self.config)
        self.period = period
        self.convs = torch.nn.ModuleList(torch.nn.ModuleList([_Conv((co, ci, k, 1), bias, use_weight_norm), _Activation()]) for ci, co, k, _, _ in geo[:-1])
        ci, co, k, _, _ = geo[-1]
        self.output_conv = _Conv((co, ci, k, 1), bias, use_weight_norm)
        self.use_weight_norm = bool(use_weight_norm)
        self._reset_cache()

    def conv_list(self):
        return [m[0] for m in self.convs] + [self.output_conv]

    def maps(self, lens):
        """kept for the next batch of the same lengths"""
        key = tuple(lens)
        plan = self.plan()
        if key != self._maps_key:
            self._maps_key, self._maps = key, PeriodMaps(plan, lens)
        return self._maps

    def forward_packed(self, x, lens):
        plan, maps = self.plan(), self.maps(lens)
        convs = self.conv_list()
        params = [m.folded() for m in convs] + ([m.bias for m in convs] if self.config["bias"] else [])
        return list(_Function.apply(plan, maps, x.index_select(0, maps.gather), *params))

    def forward(self, x, lens=None):
        x, lens = pack_input(x, lens, self.plan().device)
        return self.forward_packed(x, lens)


class HiFiGANMultiPeriodDiscriminator(_Module):
    """forward(x, lens=None) -> per period [map_0, .., map_{L-1}, scores].  Parameters: discriminators.{i}. + the period discriminator's names."""

    CHECKPOINT_KEY = "discriminator"

    def __init__(self, periods=PERIODS, discriminator_params=None):
        super().__init__()
        params = dict(discriminator_params or {})
        if "period" in params:
            raise ValueError("%s: discriminator_params=%r must not hold a period (periods gives them)" % (WHO, sorted(params)))
        if not (isinstance(periods, (tuple, list)) and len(periods) >= 1):
            raise ValueError("%s: periods=%r is not supported on the HIP path (a list of periods from 1 to 16)" % (WHO, periods))
        self.periods = tuple(periods)
        self.discriminators = torch.nn.ModuleList(HiFiGANPeriodDiscriminator(period=p, **params) for p in self.periods)
        self.use_weight_norm = self.discriminators[0].use_weight_norm
        self._reset_cache()

    def forward(self, x, lens=None):
        x, lens = pack_input(x, lens, self.discriminators[0].plan().device)
        return [d.forward_packed(x, lens) for d in self.discriminators]


def to_reference_layout(out, period, batch):
    """one period's packed outputs of a batch of `batch` equal-length utterances -> the package's views: maps [B, C, H, p], scores [B, H' p]"""
    views = []
    for a in out[:-1]:
        views.append(a.reshape(batch, period, -1, a.shape[1]).permute(0, 3, 2, 1))
    views.append(out[-1].reshape(batch, period, -1).permute(0, 2, 1).reshape(batch, -1))
    return views


def split_batch(outs, parts=2):
    """the outputs of one forward on `parts` batches of the same lengths, concatenated -> the outputs per part (utterances lie back to back at every level)"""
    return [[[torch.chunk(a, parts, 0)[i] for a in out] for out in outs] for i in range(parts)]


def generator_adversarial_loss(outs):
    """the MSE form on each period's scores, mean (p - 1)^2, averaged over the discriminators"""
    return sum(torch.mean((out[-1] - 1.0) ** 2) for out in outs) / len(outs)


def discriminator_adversarial_loss(outs_real, outs_fake):
    """-> (real loss, fake loss) = (mean (p_real - 1)^2, mean p_fake^2), each averaged over the discriminators"""
    real = sum(torch.mean((out[-1] - 1.0) ** 2) for out in outs_real) / len(outs_real)
    fake = sum(torch.mean(out[-1] ** 2) for out in outs_fake) / len(outs_fake)
    return real, fake


def feature_match_loss(feats_fake, feats_real):
    """the L1 mean per map against the detached real map, averaged over the layers and over the discriminators; the scores (last of each list) excluded"""
    total = 0.0
    for fake, real in zip(feats_fake, feats_real):
        per = sum(torch.mean(torch.abs(f - r.detach())) for f, r in zip(fake[:-1], real[:-1]))
        total = total + per / (len(fake) - 1)
    return total / len(feats_fake)
