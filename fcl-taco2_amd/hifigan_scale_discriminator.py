"""The HiFi-GAN multi-scale discriminator on the HIP path, with its backward pass, and the combined multi-scale + multi-period discriminator of the published
recipe (the hsd_* kernels of csrc/hifigan_sdisc.hip, the hpd_* kernels for the dense and the score layer).

One scale discriminator is Conv1d(1 -> channels, k0) + LeakyReLU, then per downsample scale s a grouped Conv1d(cin -> cout, k1, stride s, groups) + LeakyReLU
(widths x 2 per layer up to max_downsample_channels, groups x 4 per layer from 4 up to max_groups), a dense Conv1d(cin -> min(2 cin, max), k2) + LeakyReLU
and the score layer Conv1d(-> 1, k3) without activation, all with padding (k - 1) / 2.  It returns every activated layer's post-activation map and, last,
the scores.  The multi-scale discriminator holds `scales` of them; discriminator i sees the waveform after i AvgPool1d(4, 2, padding 2).  The published
architecture (Kong et al. 2020) as parallel_wavegan's HiFiGANScaleDiscriminator / HiFiGANMultiScaleDiscriminator /
HiFiGANMultiScaleMultiPeriodDiscriminator state it; parity with the package's checkpoints is by constructor arguments, parameter names and shapes, not
pinned against its code.

    disc = HiFiGANMultiScaleMultiPeriodDiscriminator().to("cuda:0")
    outs = disc(wave)                    # [B, T], [B, 1, T] or packed 1-D with lens= -> the scales' then the periods' [map_0 .. map_{L-1}, scores], packed
    generator_adversarial_loss(outs).backward()

The contract is stated in include/fcl_hip.h "HiFi-GAN scale discriminator" and restated in float64 numpy in tests/hfgs_ref.py.  Activations are float32,
channel-last [rows, C], the utterances back to back (to_reference_layout gives the package's [B, C, T_l] for equal lengths).  Only the post-activations
are kept for the backward pass.  Weight norm and spectral norm are folded in torch operations, so autograd carries them.  One arithmetic mode (exact
fp32).  No CPU fallback."""
import numpy as np
import torch

from . import _lib, ops
from .hfd_common import (LayerMaps, Plan, _Activation, _args, _Discriminator, _entry, _Function, activation_slope, launch_backward,  # noqa: F401
                         launch_forward, out_rows, pack_input, pack_weights, segment_tables, unpack_dweights)
from .hifigan_discriminator import (PERIODS, HiFiGANMultiPeriodDiscriminator, discriminator_adversarial_loss, feature_match_loss,  # noqa: F401
                                    generator_adversarial_loss, split_batch)
from .pwg_common import MAX_SAMPLES, _Conv, _Module

WHO = "fcl-taco2_amd: HiFi-GAN scale discriminator"
POOLING = ("AvgPool1d", {"kernel_size": 4, "stride": 2, "padding": 2})
FIRST, GROUPED, DENSE, SCORE = "first", "grouped", "dense", "score"


def check_configuration(in_channels=1, out_channels=1, kernel_sizes=(15, 41, 5, 3), channels=128, max_downsample_channels=1024, max_groups=16, bias=True,
                        downsample_scales=(2, 2, 4, 4, 1), nonlinear_activation="LeakyReLU", negative_slope=0.1, use_weight_norm=True,
                        use_spectral_norm=False):
    """-> [(cin, cout, taps, stride, pad, groups)] per layer, the score layer last; anything the kernels do not cover is refused by the argument's name"""
    bad = lambda name, got, want: ValueError("%s: %s=%r is not supported on the HIP path (%s)" % (WHO, name, got, want))
    width = lambda c: isinstance(c, int) and 16 <= c <= 1024 and c % 16 == 0
    odd = lambda k, hi: isinstance(k, int) and 3 <= k <= hi and k % 2 == 1
    if in_channels != 1:
        raise bad("in_channels", in_channels, "1")
    if out_channels != 1:
        raise bad("out_channels", out_channels, "1")
    ks = tuple(kernel_sizes) if isinstance(kernel_sizes, (tuple, list)) else ()
    if len(ks) != 4 or not odd(ks[0], 15) or not odd(ks[1], 41) or ks[2] not in (3, 5) or ks[3] != 3:
        raise bad("kernel_sizes", kernel_sizes, "(odd 3 to 15, odd 3 to 41, 3 or 5, 3)")
    if not width(channels):
        raise bad("channels", channels, "a multiple of 16 from 16 to 1024")
    if not width(max_downsample_channels):
        raise bad("max_downsample_channels", max_downsample_channels, "a multiple of 16 from 16 to 1024")
    if not (isinstance(max_groups, int) and max_groups >= 1):
        raise bad("max_groups", max_groups, "a positive integer")
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
    if use_spectral_norm not in (True, False) or (use_spectral_norm and use_weight_norm):
        raise bad("use_spectral_norm", use_spectral_norm, "True or False, and not together with use_weight_norm")
    geo = [(1, channels, ks[0], 1, (ks[0] - 1) // 2, 1)]
    ci, co, groups = channels, channels, 4
    for i, s in enumerate(sc):
        if ci % groups or co % groups or (co // groups) % 16 or (ci // groups) % 8:
            name, got = ("channels", channels) if i == 0 else ("max_groups", max_groups)
            raise bad(name, got, "layer %d (%d -> %d in %d groups) needs cout / groups a multiple of 16 and cin / groups a multiple of 8" % (i + 1, ci, co, groups))
        geo.append((ci, co, ks[1], s, (ks[1] - 1) // 2, groups))
        ci, co, groups = co, min(2 * co, max_downsample_channels), min(4 * groups, max_groups)
    co = min(2 * ci, max_downsample_channels)
    geo.append((ci, co, ks[2], 1, (ks[2] - 1) // 2, 1))
    geo.append((co, 1, ks[3], 1, (ks[3] - 1) // 2, 1))
    return geo


def layer_kinds(geometry):
    """which entries run each layer: the first and the grouped layers the hsd_* ones, the dense and the score layer the hpd_* ones"""
    return [FIRST] + [GROUPED] * (len(geometry) - 3) + [DENSE, SCORE]


def pooled_length(n):
    """AvgPool1d(4, 2, padding 2): (n + 4 - 4) // 2 + 1"""
    return n // 2 + 1


class ScalePlan(Plan):
    """Per-layer geometry (cin, cout, taps, stride, pad, groups), the score layer last, and the sizes of what a pass needs (hfd_common.Plan: heights, rows,
    act_shapes, kept_bytes, workspace_floats, dweight_shapes, slot_index); an utterance is one segment, and `kinds` says which entries run each layer"""

    period = 1

    def __init__(self, device="cuda:0", **config):
        self.geometry = check_configuration(**config)
        self.kinds = layer_kinds(self.geometry)
        self.slope, self.bias = float(config.get("negative_slope", 0.1)), bool(config.get("bias", True))
        self._on(device)

    def hsd(self, layer):
        return self.kinds[layer] in (FIRST, GROUPED)


class LayerPlan(ScalePlan):
    """one layer alone (what ScalePlan holds per layer), for launches on given inputs"""

    def __init__(self, device, cin, cout, taps, stride, pad, groups=1, slope=0.1):
        self.geometry, self.slope, self.bias, self.layers = [(cin, cout, taps, stride, pad, groups)], float(slope), True, 1
        self.kinds = [FIRST if cin == 1 else SCORE if cout == 1 else DENSE if (groups == 1 and taps <= 5) else GROUPED]
        self.device, self._slot_index = torch.device(device), {}


class ScaleMaps(object):
    """the rows of a packed batch under one scale discriminator: per layer l the int32 device tables src / in_lo / in_hi at the rate of its output rows and
    the row counts per level"""

    def __init__(self, plan, lens):
        self.lens = [int(n) for n in lens]
        if not self.lens or min(self.lens) < 1:
            raise ValueError("%s: lens=%r: every utterance needs at least one sample" % (WHO, self.lens))
        self.samples, self.n_utt = sum(self.lens), len(self.lens)
        per = np.array([plan.heights(n) for n in self.lens], dtype=np.int64)  # [utt, level]
        self.rows = [int(per[:, l].sum()) for l in range(plan.layers + 1)]
        if max(self.rows) > MAX_SAMPLES:
            raise _lib.FclError("fcl-taco2_amd: more than 2^31 rows in one scale-discriminator batch")
        self.src, self.in_lo, self.in_hi = [], [], []
        for l, (_, _, k, s, pad, _) in enumerate(plan.geometry):
            src, lo, hi = segment_tables(per[:, l], k, s, pad, plan.device)
            self.src.append(src), self.in_lo.append(lo), self.in_hi.append(hi)


class PoolMaps(object):
    """the utterances' first rows before and after one pooling: in_off / out_off [n_utt + 1] int32 on the device, and the pooled lengths"""

    def __init__(self, lens, device):
        self.lens = [int(n) for n in lens]
        if not self.lens or min(self.lens) < 1:
            raise ValueError("%s: lens=%r: every utterance needs at least one sample" % (WHO, self.lens))
        self.out_lens = [pooled_length(n) for n in self.lens]
        self.rows_in, self.rows_out, self.n_utt = sum(self.lens), sum(self.out_lens), len(self.lens)
        if self.rows_in > MAX_SAMPLES:
            raise _lib.FclError("fcl-taco2_amd: more than 2^31 samples in one scale-discriminator batch")
        off = lambda v: torch.tensor(np.concatenate([[0], np.cumsum(v)]).astype(np.int32)).to(device)
        self.in_off, self.out_off = off(self.lens), off(self.out_lens)


def launch_pool(pm, x, y, adjoint=False):
    """pm: PoolMaps.  forward: x [rows_in] -> y [rows_out]; adjoint: x = the gradient [rows_out] -> y [rows_in]"""
    lib = _lib.load()
    f = lib.fcl_hsd_pool_dx if adjoint else lib.fcl_hsd_pool_fwd
    _lib.check(f(x.data_ptr(), y.data_ptr(), pm.in_off.data_ptr(), pm.out_off.data_ptr(), pm.n_utt, pm.rows_in, pm.rows_out, ops._stream()))


class _Pool(torch.autograd.Function):
    """the average pooling between two scale discriminators, per utterance; its backward is the adjoint, so autograd sums the scales' waveform gradients"""

    @staticmethod
    def forward(ctx, pm, x):
        with torch.cuda.device(x.device):
            x = x.detach().to(torch.float32).contiguous()
            y = torch.empty(pm.rows_out, device=x.device, dtype=torch.float32)
            launch_pool(pm, x, y)
        ctx.pm = pm
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        pm = ctx.pm
        with torch.cuda.device(dy.device):
            dy = dy.detach().to(torch.float32).contiguous()
            dx = torch.empty(pm.rows_in, device=dy.device, dtype=torch.float32)
            launch_pool(pm, dy, dx, adjoint=True)
        return None, dx


class _SpectralConv(torch.nn.Module):
    """the parameters of one convolution under torch.nn.utils.spectral_norm's names: weight_orig (and bias), the buffers weight_u [cout] and
    weight_v [cin / groups x k].  folded() = weight_orig / sigma, sigma = u . (W v) on the [cout, -1] matrix; in training mode one power iteration runs
    first, under no_grad and in place; in eval mode none"""

    EPS = 1e-12

    def __init__(self, shape, bias):
        super().__init__()
        w = torch.empty(*shape)
        torch.nn.init.kaiming_normal_(w, nonlinearity="relu")
        self.weight_orig = torch.nn.Parameter(w)
        unit = lambda v: v / max(float(torch.linalg.vector_norm(v)), self.EPS)
        self.register_buffer("weight_u", unit(torch.randn(shape[0])))
        self.register_buffer("weight_v", unit(torch.randn(int(np.prod(shape[1:])))))
        self.register_parameter("bias", torch.nn.Parameter(torch.zeros(shape[0])) if bias else None)

    def folded(self):
        mat = self.weight_orig.reshape(self.weight_orig.shape[0], -1)
        if self.training:
            with torch.no_grad():
                v = torch.mv(mat.t(), self.weight_u)
                self.weight_v.copy_(v / torch.clamp(torch.linalg.vector_norm(v), min=self.EPS))
                u = torch.mv(mat, self.weight_v)
                self.weight_u.copy_(u / torch.clamp(torch.linalg.vector_norm(u), min=self.EPS))
        u, v = self.weight_u.clone(), self.weight_v.clone()
        sigma = torch.dot(u, torch.mv(mat, v))
        return self.weight_orig / sigma


class HiFiGANScaleDiscriminator(_Discriminator):
    """forward(x, lens=None) -> [map_0, .., map_{L-1}, scores], packed.  Parameters: layers.{l}.0.weight / .bias for the activated layers and
    layers.{L}.weight / .bias for the score layer (weight_g / weight_v under use_weight_norm; weight_orig with the buffers weight_u / weight_v under
    use_spectral_norm), Conv1d-shaped [cout, cin / groups, k]; Kaiming-normal weights, zero biases."""

    PLAN, MAPS = ScalePlan, ScaleMaps

    def __init__(self, in_channels=1, out_channels=1, kernel_sizes=(15, 41, 5, 3), channels=128, max_downsample_channels=1024, max_groups=16, bias=True,
                 downsample_scales=(2, 2, 4, 4, 1), nonlinear_activation="LeakyReLU", nonlinear_activation_params=None, use_weight_norm=True,
                 use_spectral_norm=False, negative_slope=None):
        super().__init__()
        slope = activation_slope(WHO, nonlinear_activation_params, negative_slope)
        self.config = dict(in_channels=in_channels, out_channels=out_channels, kernel_sizes=tuple(kernel_sizes), channels=channels,
                           max_downsample_channels=max_downsample_channels, max_groups=max_groups, bias=bias, downsample_scales=tuple(downsample_scales),
                           nonlinear_activation=nonlinear_activation, negative_slope=slope, use_weight_norm=use_weight_norm,
                           use_spectral_norm=use_spectral_norm)
        geo = check_configuration(**self.config)
        holder = (lambda shape: _SpectralConv(shape, bias)) if use_spectral_norm else (lambda shape: _Conv(shape, bias, use_weight_norm))
        layers = [torch.nn.ModuleList([holder((co, ci // gr, k)), _Activation()]) for ci, co, k, _, _, gr in geo[:-1]]
        ci, co, k, _, _, gr = geo[-1]
        self.layers = torch.nn.ModuleList(layers + [holder((co, ci // gr, k))])
        self.use_weight_norm, self.use_spectral_norm = bool(use_weight_norm), bool(use_spectral_norm)
        self._reset_cache()

    def conv_list(self):
        return [m[0] for m in list(self.layers)[:-1]] + [self.layers[-1]]


class HiFiGANMultiScaleDiscriminator(_Module):
    """forward(x, lens=None) -> per scale [map_0, .., map_{L-1}, scores]; discriminator i sees the waveform pooled i times.  Parameters:
    discriminators.{i}. + the scale discriminator's names.  follow_official_norm: discriminator 0 under spectral norm, the others under weight norm."""

    CHECKPOINT_KEY = "discriminator"

    def __init__(self, scales=3, downsample_pooling="AvgPool1d", downsample_pooling_params=None, discriminator_params=None, follow_official_norm=False):
        super().__init__()
        if not (isinstance(scales, int) and 1 <= scales <= 4):
            raise ValueError("%s: scales=%r is not supported on the HIP path (1 to 4)" % (WHO, scales))
        if downsample_pooling != POOLING[0]:
            raise ValueError("%s: downsample_pooling=%r is not supported on the HIP path (%s)" % (WHO, downsample_pooling, POOLING[0]))
        if downsample_pooling_params is not None and dict(downsample_pooling_params) != POOLING[1]:
            raise ValueError("%s: downsample_pooling_params=%r is not supported on the HIP path (%r)" % (WHO, downsample_pooling_params, POOLING[1]))
        if follow_official_norm not in (True, False):
            raise ValueError("%s: follow_official_norm=%r is not supported on the HIP path (True or False)" % (WHO, follow_official_norm))
        params = dict(discriminator_params or {})
        discs = []
        for i in range(scales):
            p = dict(params)
            if follow_official_norm:
                p["use_weight_norm"], p["use_spectral_norm"] = i != 0, i == 0
            discs.append(HiFiGANScaleDiscriminator(**p))
        self.scales = scales
        self.discriminators = torch.nn.ModuleList(discs)
        self.use_weight_norm = any(d.use_weight_norm for d in discs)
        self._reset_cache()
        self._pool_key, self._pools = None, None

    def pools(self, lens, device):
        """the offsets of every pooling, kept for the next batch of the same lengths"""
        key = (tuple(lens), str(device))
        if key != self._pool_key:
            pools, cur = [], list(lens)
            for _ in range(self.scales - 1):
                pools.append(PoolMaps(cur, device))
                cur = pools[-1].out_lens
            self._pool_key, self._pools = key, pools
        return self._pools

    def forward_packed(self, x, lens):
        pools = self.pools(lens, x.device)
        outs = []
        for i, d in enumerate(self.discriminators):
            outs.append(d.forward_packed(x, lens))
            if i + 1 < self.scales:
                x, lens = _Pool.apply(pools[i], x), pools[i].out_lens
        return outs

    def forward(self, x, lens=None):
        x, lens = pack_input(x, lens, self.discriminators[0].plan().device)
        return self.forward_packed(x, lens)


class HiFiGANMultiScaleMultiPeriodDiscriminator(_Module):
    """forward(x, lens=None) -> msd(x) + mpd(x): the scale discriminators' outputs followed by the period discriminators'; the three losses take that list
    as it is.  Parameters: msd. / mpd. + the two modules' names."""

    CHECKPOINT_KEY = "discriminator"

    def __init__(self, scales=3, scale_downsample_pooling="AvgPool1d", scale_downsample_pooling_params=None, scale_discriminator_params=None,
                 follow_official_norm=True, periods=PERIODS, period_discriminator_params=None):
        super().__init__()
        self.msd = HiFiGANMultiScaleDiscriminator(scales=scales, downsample_pooling=scale_downsample_pooling,
                                                  downsample_pooling_params=scale_downsample_pooling_params, discriminator_params=scale_discriminator_params,
                                                  follow_official_norm=follow_official_norm)
        self.mpd = HiFiGANMultiPeriodDiscriminator(periods=periods, discriminator_params=period_discriminator_params)
        self.use_weight_norm = self.msd.use_weight_norm or self.mpd.use_weight_norm
        self._reset_cache()

    def forward(self, x, lens=None):
        x, lens = pack_input(x, lens, self.msd.discriminators[0].plan().device)
        return self.msd.forward_packed(x, lens) + [d.forward_packed(x, lens) for d in self.mpd.discriminators]


def to_reference_layout(out, batch):
    """one scale's packed outputs of a batch of `batch` equal-length utterances -> the package's views: maps [B, C, T_l], scores [B, 1, T']"""
    views = [a.reshape(batch, -1, a.shape[1]).permute(0, 2, 1) for a in out[:-1]]
    return views + [out[-1].reshape(batch, 1, -1)]
