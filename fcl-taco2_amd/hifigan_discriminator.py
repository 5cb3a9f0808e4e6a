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
import numpy as np
import torch

from . import _lib, hfd_common
from .hfd_common import (LayerMaps, Plan, _Activation, _args, _Discriminator, _Function, activation_slope, launch_backward, launch_forward,  # noqa: F401
                         out_rows, pack_input, pack_weights, segment_tables)
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


class PeriodPlan(Plan):
    """Per-layer geometry (cin, cout, taps, stride, pad), the score layer last, and the sizes of what a pass needs (hfd_common.Plan: heights, rows,
    act_shapes, kept_bytes, workspace_floats, dweight_shapes, slot_index); every layer runs on the fcl_hpd_* entries, the weights are Conv2d-shaped"""

    CONV2D = True

    def __init__(self, device="cuda:0", **config):
        config = {k: v for k, v in config.items() if k != "lens"}
        self.geometry = check_configuration(**config)
        cfg = dict(period=3, negative_slope=0.1, bias=True)
        cfg.update({k: v for k, v in config.items() if k in cfg})
        self.period, self.slope, self.bias = cfg["period"], float(cfg["negative_slope"]), bool(cfg["bias"])
        self._on(device)


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


def unpack_dweights(dws):
    """the kernels' [taps, cin, cout] -> torch's [cout, cin, taps, 1]"""
    return hfd_common.unpack_dweights(dws, conv2d=True)


class HiFiGANPeriodDiscriminator(_Discriminator):
    """forward(x, lens=None) -> [map_0, .., map_{L-1}, scores], packed.  Parameters: convs.{l}.0.weight / .bias and output_conv.weight / .bias (weight_g /
    weight_v under use_weight_norm), Conv2d-shaped [cout, cin, k, 1]; Kaiming-normal weights, zero biases."""

    PLAN, MAPS = PeriodPlan, PeriodMaps

    def __init__(self, in_channels=1, out_channels=1, period=3, kernel_sizes=(5, 3), channels=32, downsample_scales=(3, 3, 3, 3, 1),
                 max_downsample_channels=1024, bias=True, nonlinear_activation="LeakyReLU", nonlinear_activation_params=None, use_weight_norm=True,
                 use_spectral_norm=False, negative_slope=None):
        super().__init__()
        slope = activation_slope(WHO, nonlinear_activation_params, negative_slope)
        self.config = dict(in_channels=in_channels, out_channels=out_channels, period=period, kernel_sizes=tuple(kernel_sizes), channels=channels,
                           downsample_scales=tuple(downsample_scales), max_downsample_channels=max_downsample_channels, bias=bias,
                           nonlinear_activation=nonlinear_activation, negative_slope=slope, use_weight_norm=use_weight_norm, use_spectral_norm=use_spectral_norm)
        geo = check_configuration(**self.config)
        self.period = period
        self.convs = torch.nn.ModuleList(torch.nn.ModuleList([_Conv((co, ci, k, 1), bias, use_weight_norm), _Activation()]) for ci, co, k, _, _ in geo[:-1])
        ci, co, k, _, _ = geo[-1]
        self.output_conv = _Conv((co, ci, k, 1), bias, use_weight_norm)
        self.use_weight_norm = bool(use_weight_norm)
        self._reset_cache()

    def conv_list(self):
        return [m[0] for m in self.convs] + [self.output_conv]


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
