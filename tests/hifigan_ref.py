"""HiFi-GAN generator: an independent float64 restatement of the published forward (kan-bayashi/ParallelWaveGAN `HiFiGANGenerator`), the seeded random
state dicts and inputs of its tests, and the float32 torch module of tools/hifigan_ab.py.  Plain torch; nothing here calls a kernel of the library or
reads fcl_taco2_amd/hifigan.py (the transposed convolution is torch.nn.functional.conv_transpose1d, not the package's index rule).

Layout as on the device: rows are samples (or frames), channels are columns; every function sees ONE utterance, so its edges are real zero padding.
tests/test_hifigan_cpu.py checks the input conditions with these functions alone; tests/test_gpu_hifigan.py runs the very same arrays on the device."""
import math

import numpy as np
import torch
import torch.nn.functional as F

V1 = dict(in_channels=80, out_channels=1, channels=512, kernel_size=7, upsample_scales=(8, 8, 2, 2), upsample_kernel_sizes=(16, 16, 4, 4),
          resblock_kernel_sizes=(3, 7, 11), resblock_dilations=((1, 3, 5), (1, 3, 5), (1, 3, 5)), negative_slope=0.1)
# the kernels need every stage's width to be a multiple of 32: 128 channels over two stages give 64 and 32
SMALL = dict(V1, channels=128, upsample_scales=(4, 2), upsample_kernel_sizes=(8, 4))
OUT_SLOPE = 0.01  # torch.nn.LeakyReLU()'s default: the package's output stage does not pass negative_slope

# whole-generator seeds: the first seed from 5 up whose batch (GENERATOR_LENS) meets the input conditions of tests/test_hifigan_cpu.py with this module's
# draw order -- found with the reference alone (v1: seed 5 peaks at |pre-tanh| = 4.96 on the 70-frame batch, seed 6 at 2.68)
SEEDS = dict(v1=6, small=5, tconv=11, unit=12, out=13, bf16=14, drivers=15)
GENERATOR_LENS = [29, 3, 1, 33, 2, 2]  # frames per utterance of the whole-generator tests
CONDITION_LENS = dict(v1=[9], small=[37])  # the single utterances the input conditions are asserted on (test_hifigan_cpu.py)


def plan_cfg(cfg):
    """cfg of this module -> the overrides fcl_taco2_amd.hifigan.config takes"""
    c = {k: v for k, v in cfg.items() if k != "negative_slope"}
    c["nonlinear_activation_params"] = dict(negative_slope=cfg["negative_slope"])
    return c


def param_shapes(cfg):
    """Ordered {state-dict name: (shape, fan_in)} from the published constructor (weight norm folded)."""
    ch, k, nk = cfg["channels"], cfg["kernel_size"], len(cfg["resblock_kernel_sizes"])
    out = {"input_conv.weight": ((ch, cfg["in_channels"], k), cfg["in_channels"] * k), "input_conv.bias": ((ch,), None)}
    for i, (s, ku) in enumerate(zip(cfg["upsample_scales"], cfg["upsample_kernel_sizes"])):
        ci, co = ch >> i, ch >> (i + 1)
        out["upsamples.%d.1.weight" % i] = ((ci, co, ku), ci * ku // s)  # ConvTranspose1d: (in, out, k); ku / s taps meet one output sample
        out["upsamples.%d.1.bias" % i] = ((co,), None)
        for j, kr in enumerate(cfg["resblock_kernel_sizes"]):
            for d in range(len(cfg["resblock_dilations"][j])):
                for cv in ("convs1", "convs2"):
                    p = "blocks.%d.%s.%d.1." % (i * nk + j, cv, d)
                    out[p + "weight"], out[p + "bias"] = ((co, co, kr), co * kr), ((co,), None)
    cl = ch >> len(cfg["upsample_scales"])
    out["output_conv.1.weight"], out["output_conv.1.bias"] = ((cfg["out_channels"], cl, k), cl * k), ((cfg["out_channels"],), None)
    return out


def random_state_dict(rng, cfg):
    """weights N(0, 1 / fan_in), biases N(0, 1 / 4); float32 numpy arrays"""
    sd = {}
    for k, (shp, fan_in) in param_shapes(cfg).items():
        v = 0.5 * rng.standard_normal(shp) if fan_in is None else rng.standard_normal(shp) / math.sqrt(fan_in)
        sd[k] = np.ascontiguousarray(v, dtype=np.float32)
    return sd


def generator_inputs(seed, lens, cfg):
    """(state dict, mels) of the whole-generator tests: random_state_dict, mel N(0, 1)"""
    rng = np.random.RandomState(seed)
    sd = random_state_dict(rng, cfg)
    return sd, [rng.standard_normal((n, cfg["in_channels"])).astype(np.float32) for n in lens]


def with_weight_norm(sd, rng):
    """the same generator as a checkpoint stores it: weight_g / weight_v with v at a random scale per output row (dim 0)"""
    out = {}
    for k, v in sd.items():
        if k.endswith("weight"):
            scale = np.exp(rng.standard_normal((v.shape[0],) + (1,) * (v.ndim - 1))).astype(np.float32)
            vv = (v * scale).astype(np.float32)
            out[k + "_g"] = np.sqrt((vv.astype(np.float64).reshape(v.shape[0], -1) ** 2).sum(1)).reshape(scale.shape).astype(np.float32) / scale
            out[k + "_v"] = vv
        else:
            out[k] = v
    return out


def f64(a):
    return torch.from_numpy(np.asarray(a)).to(torch.float64) if not torch.is_tensor(a) else a.to(torch.float64)


def plane_round(t):
    """the value the P32 planes of a float32 number carry (hi + lo), as float64"""
    x = t.to(torch.float32)
    hi = x.to(torch.bfloat16).to(torch.float32)
    lo = (x - hi).to(torch.bfloat16).to(torch.float32)
    return hi.to(torch.float64) + lo.to(torch.float64)


def bf16_round(t):
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def lrelu(x, slope):
    return torch.where(x >= 0, x, x * slope)


def shift(x, sh):
    """rows t -> x[t + sh], zero where t + sh leaves the utterance"""
    out = torch.zeros_like(x)
    n = x.shape[0]
    if sh >= 0:
        if sh < n:
            out[: n - sh] = x[sh:]
    elif -sh < n:
        out[-sh:] = x[: n + sh]
    return out


def conv1d(x_op, w, b, dilation=1, rnd_w=None):
    """Conv1d with 'same' zero padding on one utterance: x_op [T, Cin] (the operand as the GEMM sees it), w (Cout, Cin, k) -> [T, Cout]"""
    k = w.shape[2]
    rw = rnd_w or (lambda t: t)
    y = b.clone().expand(x_op.shape[0], -1).clone()
    for j in range(k):
        y = y + shift(x_op, (j - (k - 1) // 2) * dilation) @ rw(w[:, :, j]).t()
    return y


def tconv(x_op, w, b, s, rnd_w=None):
    """ConvTranspose1d(stride s, padding s // 2 + s % 2, output_padding s % 2) on one utterance: x_op [T, Cin], w (Cin, Cout, ku) -> [T * s, Cout]"""
    rw = rnd_w or (lambda t: t)
    y = F.conv_transpose1d(x_op.t().unsqueeze(0), rw(w), b, stride=s, padding=s // 2 + s % 2, output_padding=s % 2)
    assert y.shape[2] == x_op.shape[0] * s, (y.shape, x_op.shape, s)
    return y[0].t().contiguous()


def unit(x, w1, b1, w2, b2, dilation, slope, rnd=None):
    """one residual unit on one utterance; returns (x + conv2(lrelu(conv1(lrelu(x)))), the intermediate xt)"""
    r = rnd or (lambda t: t)
    xt = conv1d(r(lrelu(x, slope)), w1, b1, dilation, rnd)
    return conv1d(r(lrelu(xt, slope)), w2, b2, 1, rnd) + x, xt


def generator_f64(sd, mel, cfg, rnd=None, rnd_out_w=None, zero_unit=None):
    """The whole generator on ONE utterance in float64: mel [T', in].  rnd: rounding applied to every GEMM operand (activations after their
    LeakyReLU, the mel, weights) -- the operand-format error model; None = exact.  rnd_out_w: rounding of output_conv's weights (the row-wise output
    kernel keeps them in fp32 unless the bf16 mode is on).  zero_unit = (stage, block, unit): that unit contributes nothing (x passes through).
    Returns c0 (input_conv), stages (c after every stage), pre (output_conv before tanh), wav [T' * hop, out] and lrelu_args (every tensor a
    LeakyReLU is applied to)."""
    r = rnd or (lambda t: t)
    t = lambda k: f64(sd[k])
    slope, nk = cfg["negative_slope"], len(cfg["resblock_kernel_sizes"])
    args = []
    c = conv1d(r(f64(mel)), t("input_conv.weight"), t("input_conv.bias"), 1, rnd)
    c0, stages = c, []
    for i, s in enumerate(cfg["upsample_scales"]):
        args.append(c)
        c = tconv(r(lrelu(c, slope)), t("upsamples.%d.1.weight" % i), t("upsamples.%d.1.bias" % i), s, rnd)
        cs = 0
        for j in range(nk):
            x = c
            for d, dil in enumerate(cfg["resblock_dilations"][j]):
                if zero_unit == (i, j, d):
                    continue
                p = "blocks.%d." % (i * nk + j)
                args.append(x)
                x, xt = unit(x, t(p + "convs1.%d.1.weight" % d), t(p + "convs1.%d.1.bias" % d), t(p + "convs2.%d.1.weight" % d),
                             t(p + "convs2.%d.1.bias" % d), dil, slope, rnd)
                args.append(xt)
            cs = cs + x
        c = cs / nk
        stages.append(c)
    args.append(c)
    pre = conv1d(r(lrelu(c, OUT_SLOPE)), t("output_conv.1.weight"), t("output_conv.1.bias"), 1, rnd_out_w)
    return dict(c0=c0, stages=stages, pre=pre, wav=torch.tanh(pre), lrelu_args=args)


def units_of(cfg):
    nk = len(cfg["resblock_kernel_sizes"])
    return [(i, j, d) for i in range(len(cfg["upsample_scales"])) for j in range(nk) for d in range(len(cfg["resblock_dilations"][j]))]


def taps_of(res):
    """what HiFiGANGenerator.synthesize_packed(return_intermediates=True) returns as `taps`, from generator_f64's result"""
    return [res["c0"]] + list(res["stages"])


def bound(e_model, peak):
    """the project's whole-generator bound (test_generator_v1_every_tap_vs_float64): 4 x max(operand-format model error, plane storage 2^-15 peak)"""
    return 4 * max(e_model, 2.0 ** -15 * peak)


# ---- the single-kernel cases ------------------------------------------------------------------------------------------------------------------
TCONV_SCALES, TCONV_CIN = (2, 4, 8), (64, 128, 512)
TCONV_LENS = [[1], [3, 1, 7, 2], [40, 1, 130]]  # input rows per utterance: a one-row utterance, ragged lists, an edge inside a 128-row tile
UNIT_KERNELS, UNIT_DILATIONS, UNIT_CHANNELS = (3, 7, 11), (1, 3, 5), (32, 64, 128, 256)
UNIT_LENS = [[1, 2, 5], [20, 1, 100, 7, 130]]  # rows: utterances shorter than the 25-row halo, edges inside a 112-row tile, more than one tile


def tconv_case(seed, s, cin, lens):
    """(x [sum lens, cin] = N(0, 1), w (cin, cin / 2, 2 s), b) float32"""
    rng = np.random.RandomState(seed + 1000 * s + cin + sum(lens))
    cout, ku = cin // 2, 2 * s
    f = lambda *shp: rng.standard_normal(shp).astype(np.float32)
    return f(sum(lens), cin), (f(cin, cout, ku) / np.float32(math.sqrt(cin * ku // s))), np.float32(0.5) * f(cout)


def unit_case(seed, kr, dil, c, lens):
    """(x [sum lens, c] = N(0, 1), w1, b1, w2, b2, cs0 [sum lens, c] = N(0, 1)) float32"""
    rng = np.random.RandomState(seed + 100 * kr + 10 * dil + c + sum(lens))
    f = lambda *shp: rng.standard_normal(shp).astype(np.float32)
    g = np.float32(1.0 / math.sqrt(c * kr))
    return f(sum(lens), c), f(c, c, kr) * g, np.float32(0.5) * f(c), f(c, c, kr) * g, np.float32(0.5) * f(c), f(sum(lens), c)


class TorchHiFiGAN(torch.nn.Module):
    """the float32 torch module of the same architecture (channels-first, batch of one utterance): the eager leg of tools/hifigan_ab.py"""

    def __init__(self, sd, cfg):
        super().__init__()
        self.cfg = cfg
        for k, v in sd.items():
            self.register_buffer(k.replace(".", "_"), torch.from_numpy(np.asarray(v, dtype=np.float32)))

    def p(self, k):
        return getattr(self, k.replace(".", "_"))

    def forward(self, mel):
        """mel [B, in, T] -> [B, out, T * hop]"""
        cfg = self.cfg
        slope, nk, k = cfg["negative_slope"], len(cfg["resblock_kernel_sizes"]), cfg["kernel_size"]
        c = F.conv1d(mel, self.p("input_conv.weight"), self.p("input_conv.bias"), padding=(k - 1) // 2)
        for i, s in enumerate(cfg["upsample_scales"]):
            c = F.conv_transpose1d(F.leaky_relu(c, slope), self.p("upsamples.%d.1.weight" % i), self.p("upsamples.%d.1.bias" % i), stride=s,
                                   padding=s // 2 + s % 2, output_padding=s % 2)
            cs = None
            for j, kr in enumerate(cfg["resblock_kernel_sizes"]):
                x = c
                for d, dil in enumerate(cfg["resblock_dilations"][j]):
                    p = "blocks.%d." % (i * nk + j)
                    xt = F.conv1d(F.leaky_relu(x, slope), self.p(p + "convs1.%d.1.weight" % d), self.p(p + "convs1.%d.1.bias" % d), dilation=dil,
                                  padding=(kr - 1) // 2 * dil)
                    xt = F.conv1d(F.leaky_relu(xt, slope), self.p(p + "convs2.%d.1.weight" % d), self.p(p + "convs2.%d.1.bias" % d), padding=(kr - 1) // 2)
                    x = xt + x
                cs = x if cs is None else cs + x
            c = cs / nk
        return torch.tanh(F.conv1d(F.leaky_relu(c, OUT_SLOPE), self.p("output_conv.1.weight"), self.p("output_conv.1.bias"), padding=(k - 1) // 2))
