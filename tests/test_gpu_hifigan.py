"""-m gpu: every kernel of the HiFi-GAN stage (csrc/hifigan.hip) on its own and the whole generator against the float64 restatement of
tests/hifigan_ref.py (plain torch, ONE utterance at a time, so utterance edges are real zero padding).  Every buffer a kernel writes sits between
guard zones filled with a NaN bit pattern, which must survive; every test reads the library's launch record and fails if its kernel did not run.
Bounds come from the float64 reference and the project's bound for one pre-split GEMM (3e-5 x max(1, max|y|), test_gpu_planes.py; 2e-5 on
bf16-rounded operands in FCL_GEMM_BF16); tests/test_hifigan_cpu.py asserts that the inputs exercise the generator.  DESIGN.md 6c has the figures.

  1 fcl_hfg_tconv_fwd      2 fcl_hfg_unit_fwd (one launch for C <= 128, one launch per convolution for 256)      3 fcl_hfg_conv_fwd
  4 fcl_hfg_out_fwd + fcl_pcm16_fwd      5 the whole generator      6 FCL_GEMM_BF16      7 refusals      8 drivers"""
import contextlib
import ctypes as C
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

import hifigan_ref as R
from conftest import ROOT
from helpers import bf16_to_f32, max_abs, split_planes_np

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAT16, PAT32 = 0x7FC1, 0x7FC12345  # a bf16 / an fp32 NaN: whatever is read from an unwritten line poisons the result
GEMM, BF16_GEMM = 3e-5, 2e-5
SLOPE = 0.1


@pytest.fixture(scope="module")
def hfg():
    assert torch.cuda.is_available()
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib, hifigan, ops

    _lib.load()
    if not ops.planes_enabled():
        pytest.skip("FCL_PRECISION=0 / FCL_PLANES=0: the vocoder needs the pre-split operand path")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    return hifigan


def lib():
    from fcl_taco2_amd import _lib

    return _lib.load()


def chk(rc):
    from fcl_taco2_amd import _lib

    _lib.check(rc)


def stream():
    from fcl_taco2_amd import ops

    return ops._stream()


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


@contextlib.contextmanager
def launched(*names):
    """the launches inside run the named kernels (the library's own launch record)"""
    from fcl_taco2_amd import _lib

    _lib.prof_enable(True)
    try:
        yield
        torch.cuda.synchronize()
        seen = set(_lib.prof_collect())
    finally:
        _lib.prof_enable(False)
    for n in names:
        assert n in seen, (n, sorted(seen))


class Guarded(object):
    """a device buffer of n elements between two guard zones; everything starts as the NaN pattern"""

    PAD = 8192

    def __init__(self, n, dtype):
        self.n, self.dtype = int(n), dtype
        self.buf = torch.empty(self.n + 2 * self.PAD, dtype=dtype, device=DEV)
        self.bits().fill_(PAT16 if dtype == torch.int16 else PAT32)
        assert self.t.data_ptr() % 128 == 0

    def bits(self):
        return self.buf if self.dtype == torch.int16 else self.buf.view(torch.int32)

    @property
    def t(self):
        return self.buf[self.PAD : self.PAD + self.n]

    def intact(self):
        b, p = self.bits(), PAT16 if self.dtype == torch.int16 else PAT32
        return bool((b[: self.PAD] == p).all()) and bool((b[self.PAD + self.n :] == p).all())


def lrelu32(x, slope):
    """LeakyReLU as the kernels evaluate it, in float32"""
    x = np.asarray(x, dtype=np.float32)
    return np.where(x >= 0, x, x * np.float32(slope)).astype(np.float32)


def planes_of(g, rows):
    """Guarded planes -> uint16 [rows, L, 2, 32]"""
    return g.t.cpu().numpy().view(np.uint16).reshape(rows, -1, 2, 32)


def tables(lens):
    """frame_utt / utt_off with one row per 'frame' (rate 1)"""
    return dev(np.repeat(np.arange(len(lens)), lens).astype(np.int32)), dev(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32))


def taps_planes(w):
    """(Cout, Cin, k) float32 -> the planes the entry points take: tap-major [k * Cout, Cin]"""
    from fcl_taco2_amd import ops

    wd = dev(w)
    return ops.pack_planes(ops.pack_conv1d_weight(wd).reshape(w.shape[2] * w.shape[0], w.shape[1]))


def operand_planes(x32):
    from fcl_taco2_amd import ops

    return ops.pack_planes(dev(x32))


def per_utt(fn, x, lens):
    out, off = [], 0
    for n in lens:
        out.append(fn(x[off : off + n]))
        off += n
    return out


@contextlib.contextmanager
def mode(name):
    from fcl_taco2_amd import ops

    if name == "bf16":
        with ops.gemm_mode("bf16"):
            yield "/bf16"
    else:
        yield ""


# ------------------------------------------------------------------------------------------------------------------ 1 transposed stage
def run_tconv(x, w, b, s, lens, padding=None, ksize=None):
    from fcl_taco2_amd import _lib

    cin, cout, ku = w.shape
    rows_in, rows_out = x.shape[0], x.shape[0] * s
    fu, uo = tables(lens)
    xp, wp, bd = operand_planes(x), taps_planes(np.ascontiguousarray(np.transpose(w, (1, 0, 2)))), dev(b)
    y, yp = Guarded(rows_out * cout, torch.float32), Guarded(rows_out * (cout // 32) * 64, torch.int16)
    a = _lib.HfgTconv()
    a.m_in, a.cin, a.cout, a.stride, a.ksize, a.rate_in, a.slope = rows_in, cin, cout, s, ku if ksize is None else ksize, 1, SLOPE
    a.padding = s // 2 + s % 2 if padding is None else padding
    a.xp, a.wp, a.bias, a.frame_utt, a.utt_off, a.y, a.yp = xp.data_ptr(), wp.data_ptr(), bd.data_ptr(), fu.data_ptr(), uo.data_ptr(), y.t.data_ptr(), yp.t.data_ptr()
    rc = lib().fcl_hfg_tconv_fwd(C.byref(a), stream())
    torch.cuda.synchronize()
    return rc, y, yp


@pytest.mark.parametrize("cin", R.TCONV_CIN)
@pytest.mark.parametrize("s", R.TCONV_SCALES)
def test_tconv_stage_vs_float64(hfg, s, cin):
    """values within the per-GEMM bound of torch's float64 conv_transpose1d per utterance; planes = the split of LeakyReLU(fp32 value), bit for bit"""
    for lens in R.TCONV_LENS:
        x, w, b = R.tconv_case(R.SEEDS["tconv"], s, cin, lens)
        ref = torch.cat(per_utt(lambda xs: R.tconv(R.f64(xs), R.f64(w), R.f64(b), s), x, lens)).numpy()
        with launched("hfg_tconv_kernel"):
            rc, y, yp = run_tconv(x, w, b, s, lens)
            chk(rc)
        rows = x.shape[0] * s
        got = y.t.reshape(rows, -1).cpu().numpy()
        err, tol = max_abs(got, ref), GEMM * max(1.0, float(np.abs(ref).max()))
        print("tconv s=%d cin=%d lens=%r: err %.3e bound %.3e" % (s, cin, lens, err, tol))
        assert err <= tol, (lens, err, tol)
        assert np.array_equal(planes_of(yp, rows), split_planes_np(lrelu32(got, SLOPE))), lens
        assert y.intact() and yp.intact()


# ------------------------------------------------------------------------------------------------------------------ 2 residual unit
def run_unit(case, kr, dil, lens, variant, kernel_suffix=""):
    """variant: 'mid' (x_out + xp_out), 'first' (last unit of block 0: cs written over NaN), 'acc' (last unit of the last block: cs accumulated, csp)"""
    from fcl_taco2_amd import _lib, ops

    x, w1, b1, w2, b2, cs0 = case
    m, c = x.shape
    fu, uo = tables(lens)
    xd, xp = dev(x), operand_planes(lrelu32(x, SLOPE))
    w1p, w2p, b1d, b2d = taps_planes(w1), taps_planes(w2), dev(b1), dev(b2)
    ld = c // 32
    out = dict(x=Guarded(m * c, torch.float32), xp=Guarded(m * ld * 64, torch.int16), cs=Guarded(m * c, torch.float32), csp=Guarded(m * ld * 64, torch.int16))
    tp = Guarded(m * ld * 64, torch.int16) if c > 128 else None
    u = _lib.HfgUnit()
    u.m, u.c, u.ksize, u.dilation, u.rate = m, c, kr, dil, 1
    u.slope, u.cs_scale, u.csp_slope = SLOPE, 1.0 / 3, R.OUT_SLOPE
    u.xp, u.x, u.w1p, u.b1, u.w2p, u.b2, u.frame_utt, u.utt_off = xp.data_ptr(), xd.data_ptr(), w1p.data_ptr(), b1d.data_ptr(), w2p.data_ptr(), b2d.data_ptr(), \
        fu.data_ptr(), uo.data_ptr()
    u.tp = None if tp is None else tp.t.data_ptr()
    u.x_out, u.xp_out = out["x"].t.data_ptr(), out["xp"].t.data_ptr()
    if variant != "mid":
        u.last, u.first = 1, int(variant == "first")
        u.cs = out["cs"].t.data_ptr()
        if variant == "acc":
            out["cs"].t.copy_(dev(cs0).reshape(-1))
            u.csp = out["csp"].t.data_ptr()
    kernel = ("hfg_unit_kernel<%d>" % c if c <= 128 else "hfg_conv_kernel") + kernel_suffix
    with launched(kernel):
        chk(lib().fcl_hfg_unit_fwd(C.byref(u), stream()))
    for g in list(out.values()) + ([tp] if tp is not None else []):
        assert g.intact()
    return out


def unit_reference(case, dil, lens, rnd=None):
    x, w1, b1, w2, b2, _ = case
    outs = per_utt(lambda xs: R.unit(R.f64(xs), R.f64(w1), R.f64(b1), R.f64(w2), R.f64(b2), dil, SLOPE, rnd), x, lens)
    return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])


def check_unit_outputs(out, got_x, case, variant, tol, lens):
    """the planes, the stage sum and its planes, given the fp32 x' the kernel wrote (itself checked against float64 by the caller)"""
    m, c = got_x.shape
    assert np.array_equal(planes_of(out["xp"], m), split_planes_np(lrelu32(got_x, SLOPE))), (variant, lens)
    if variant == "mid":
        assert bool((out["cs"].bits() == PAT32).all()) and bool((out["csp"].bits() == PAT16).all())  # not the last unit: the stage sum is not touched
        return
    cs = out["cs"].t.reshape(m, c).cpu().numpy()
    want = got_x.astype(np.float64) / 3 + (0.0 if variant == "first" else case[5].astype(np.float64))
    e = max_abs(cs, want)
    assert e <= 2.0 ** -22 * max(1.0, float(np.abs(want).max())), (variant, e)  # two fp32 roundings of the kernel's own x'
    if variant == "acc":
        assert np.array_equal(planes_of(out["csp"], m), split_planes_np(lrelu32(cs, R.OUT_SLOPE))), lens
    else:
        assert bool((out["csp"].bits() == PAT16).all())


@pytest.mark.parametrize("c", R.UNIT_CHANNELS)
@pytest.mark.parametrize("dil", R.UNIT_DILATIONS)
@pytest.mark.parametrize("kr", R.UNIT_KERNELS)
def test_residual_unit_vs_float64(hfg, kr, dil, c):
    """x' within conv1's bound carried through conv2's row-wise |W|_1 (LeakyReLU is 1-Lipschitz) plus conv2's own bound; the planes and the stage sum
    follow from the kernel's own fp32 x' exactly.  Utterances shorter than the halo, edges inside a tile, first = 1 over a NaN-filled cs."""
    for lens in R.UNIT_LENS:
        case = R.unit_case(R.SEEDS["unit"], kr, dil, c, lens)
        ref_x, ref_xt = unit_reference(case, dil, lens)
        conv2 = ref_x - R.f64(case[0])
        w2_l1 = float(np.abs(case[3].astype(np.float64)).sum(axis=(1, 2)).max())
        tol = GEMM * max(1.0, float(ref_xt.abs().max())) * w2_l1 + GEMM * max(1.0, float(conv2.abs().max()))
        for variant in ("mid", "first", "acc"):
            out = run_unit(case, kr, dil, lens, variant)
            got = out["x"].t.reshape(case[0].shape).cpu().numpy()
            err = max_abs(got, ref_x.numpy())
            print("unit kr=%d d=%d C=%d lens=%r %s: err %.3e bound %.3e" % (kr, dil, c, lens, variant, err, tol))
            assert err <= tol, (lens, variant, err, tol)
            check_unit_outputs(out, got, case, variant, tol, lens)


# ------------------------------------------------------------------------------------------------------------------ 3 single convolution
def run_conv(x_op, w, b, dil, lens, resid=None):
    from fcl_taco2_amd import _lib

    m, cin = x_op.shape
    cout, k = w.shape[0], w.shape[2]
    fu, uo = tables(lens)
    xp, wp, bd = operand_planes(x_op), taps_planes(w), dev(b)
    y, yp = Guarded(m * cout, torch.float32), Guarded(m * (cout // 32) * 64, torch.int16)
    rd = None if resid is None else dev(resid)
    a = _lib.HfgConv()
    a.m, a.cin, a.cout, a.ksize, a.dilation, a.rate, a.slope = m, cin, cout, k, dil, 1, SLOPE
    a.xp, a.wp, a.bias, a.frame_utt, a.utt_off, a.y, a.yp = xp.data_ptr(), wp.data_ptr(), bd.data_ptr(), fu.data_ptr(), uo.data_ptr(), y.t.data_ptr(), yp.t.data_ptr()
    a.resid = None if rd is None else rd.data_ptr()
    chk(lib().fcl_hfg_conv_fwd(C.byref(a), stream()))
    torch.cuda.synchronize()
    return y, yp


@pytest.mark.parametrize("cin,cout", [(80, 512), (80, 128), (96, 32)])
def test_single_conv_vs_float64(hfg, cin, cout):
    """input_conv's shape (80 channels: three lines per row, zero past 80) and a residual operand"""
    rng = np.random.RandomState(R.SEEDS["unit"] + cin + cout)
    for lens in ([1, 2, 5], [20, 1, 100, 7, 130]):
        m = sum(lens)
        x = rng.standard_normal((m, cin)).astype(np.float32)
        w = (rng.standard_normal((cout, cin, 7)) / np.sqrt(cin * 7)).astype(np.float32)
        b, resid = (0.5 * rng.standard_normal(cout)).astype(np.float32), rng.standard_normal((m, cout)).astype(np.float32)
        ref = torch.cat(per_utt(lambda xs: R.conv1d(R.f64(xs), R.f64(w), R.f64(b)), x, lens))
        tol = GEMM * max(1.0, float(ref.abs().max()))
        for rs in (None, resid):
            with launched("hfg_conv_kernel"):
                y, yp = run_conv(x, w, b, 1, lens, rs)
            got = y.t.reshape(m, cout).cpu().numpy()
            want = ref.numpy() + (0.0 if rs is None else rs.astype(np.float64))
            err = max_abs(got, want)
            assert err <= tol + 2.0 ** -23 * float(np.abs(want).max()), (lens, err, tol)
            assert np.array_equal(planes_of(yp, m), split_planes_np(lrelu32(got, SLOPE)))
            assert y.intact() and yp.intact()


# ------------------------------------------------------------------------------------------------------------------ 4 output stage
def run_out(a32, w, b, lens):
    from fcl_taco2_amd import ops

    m, c = a32.shape
    cout, k = w.shape[0], w.shape[2]
    fu, uo = tables(lens)
    ap, wd, bd = operand_planes(a32), ops.pack_conv1d_weight(dev(w)), dev(b)
    wav = Guarded(m * cout, torch.float32)
    chk(lib().fcl_hfg_out_fwd(ap.data_ptr(), wd.data_ptr(), bd.data_ptr(), fu.data_ptr(), uo.data_ptr(), 1, wav.t.data_ptr(), m, c, cout, k, stream()))
    torch.cuda.synchronize()
    return wav


@pytest.mark.parametrize("c,cout", [(32, 1), (64, 2)])
def test_output_conv_tanh_and_pcm16(hfg, c, cout):
    """fp32 FMA chain over the C k products of the operand planes' values: n 2^-24 sum|a||w| (n = C k + 8: the chain and the lane reduction) + tanhf;
    the PCM conversion of the result is the numpy rule, bit for bit"""
    from fcl_taco2_amd import vocoder

    rng = np.random.RandomState(R.SEEDS["out"] + c)
    lens = [1, 2, 40, 3, 300]
    m = sum(lens)
    a32 = lrelu32(rng.standard_normal((m, c)).astype(np.float32), R.OUT_SLOPE)
    w = (rng.standard_normal((cout, c, 7)) / np.sqrt(c * 7)).astype(np.float32)  # pre-tanh std ~0.8: tanh hides nothing
    b = (0.5 * rng.standard_normal(cout)).astype(np.float32)
    av = R.plane_round(R.f64(a32))
    pre = torch.cat(per_utt(lambda xs: R.conv1d(xs, R.f64(w), R.f64(b)), av, lens))
    mag = torch.cat(per_utt(lambda xs: R.conv1d(xs.abs(), R.f64(w).abs(), R.f64(b).abs()), av, lens))
    tol = (c * 7 + 8) * 2.0 ** -24 * float(mag.max()) + 2.0 ** -21
    with launched("hfg_out_kernel"):
        wav = run_out(a32, w, b, lens)
    got = wav.t.reshape(m, cout).cpu().numpy()
    err = max_abs(got, torch.tanh(pre).numpy())
    print("output conv C=%d: err %.3e bound %.3e, pre-tanh peak %.2f" % (c, err, tol, float(pre.abs().max())))
    assert err <= tol and wav.intact()
    with launched("pwg_pcm16_kernel"):
        pcm = vocoder.pcm16(wav.t)
    assert np.array_equal(pcm, vocoder.pcm16_rule(got.reshape(-1)))


# ------------------------------------------------------------------------------------------------------------------ 5 whole generator
def make_generator(hfg, key):
    cfg = dict(v1=R.V1, small=R.SMALL)[key]
    sd, mels = R.generator_inputs(R.SEEDS[key], R.GENERATOR_LENS, cfg)
    return cfg, sd, mels, hfg.HiFiGANGenerator(hfg.HiFiGANPlan(sd, DEV, R.plan_cfg(cfg)))


@pytest.mark.parametrize("key", ["small", "v1"])
def test_generator_every_stage_vs_float64(hfg, key):
    """input_conv's output, every stage's c and the waveform of a ragged batch with a one-frame utterance against float64;
    err <= 4 x max(error of the float64 generator on plane-rounded operands, plane storage 2^-15 max|tap|).  The batch equals per-utterance runs
    bit for bit (no padding leaks), and synthesize == synthesize_packed == inference."""
    cfg, sd, mels, gen = make_generator(hfg, key)
    kernels = ["hfg_conv_kernel", "hfg_tconv_kernel", "hfg_out_kernel", "hfg_unit_kernel<32>", "hfg_unit_kernel<64>"] + (["hfg_unit_kernel<128>"] if key == "v1" else [])
    with launched(*kernels):
        wavs, aux = gen.synthesize(mels, return_intermediates=True)
    hop = int(np.prod(cfg["upsample_scales"]))
    assert gen.plan.hop == hop and [w.shape[0] for w in wavs] == [n * hop for n in R.GENERATOR_LENS]
    refs = [R.generator_f64(sd, m, cfg) for m in mels]
    mods = [R.generator_f64(sd, m, cfg, rnd=R.plane_round) for m in mels]
    bad = []
    for l, tap in enumerate(aux["taps"]):
        t_ref = torch.cat([R.taps_of(r)[l] for r in refs])
        t_mod = torch.cat([R.taps_of(r)[l] for r in mods])
        e_gpu, e_mod = max_abs(tap.cpu().double(), t_ref), max_abs(t_mod, t_ref)
        bound = R.bound(e_mod, float(t_ref.abs().max()))
        print("%s tap %d: err_gpu %.3e err_model %.3e bound %.3e" % (key, l, e_gpu, e_mod, bound))
        if not e_gpu <= bound:
            bad.append((l, e_gpu, bound))
    for g, r, mo in zip(wavs, refs, mods):
        peak = float(r["wav"].abs().max())
        e, em = max_abs(g.cpu().double().reshape(-1, 1), r["wav"]), max_abs(mo["wav"], r["wav"])
        print("%s waveform: err_gpu %.3e err_model %.3e bound %.3e peak %.3f" % (key, e, em, R.bound(em, peak), peak))
        if not e <= R.bound(em, peak):
            bad.append(("wav", e, R.bound(em, peak)))
    assert not bad, bad
    packed = gen.synthesize_packed(torch.cat([dev(m) for m in mels]), R.GENERATOR_LENS, seed=123)
    for m, w, p in zip(mels, wavs, packed):
        one = gen.synthesize([m])[0]
        assert torch.equal(one, w) and torch.equal(p, w)
        assert torch.equal(gen.inference(m), w.reshape(-1, 1))


# ------------------------------------------------------------------------------------------------------------------ 6 FCL_GEMM_BF16
def test_bf16_mode_of_every_kernel(hfg):
    """hi planes only: every kernel against float64 on bf16-rounded operands at 2e-5 x scale per GEMM, and more than 1e-4 x scale away from the
    default-mode result.  The residual unit rounds its intermediate to bf16 between its two GEMMs, and a rounding is discontinuous, so the rounding is
    made observable: conv1 runs through fcl_hfg_conv_fwd in bf16 mode (2e-5 x scale against float64), the hi plane it WROTE is read back, conv2 runs
    on exactly those bf16 values (2e-5 x scale against float64 on the same values), and the unit kernel -- fused, or one launch per convolution at
    256 channels -- must equal that two-launch result within one GEMM bound."""
    from fcl_taco2_amd import _lib

    rb = R.bf16_round
    # transposed stage
    s, cin, lens = 4, 128, R.TCONV_LENS[2]
    x, w, b = R.tconv_case(R.SEEDS["bf16"], s, cin, lens)
    ref = torch.cat(per_utt(lambda xs: R.tconv(rb(R.f64(xs)), R.f64(w), R.f64(b), s, rb), x, lens)).numpy()
    rc, y0, _ = run_tconv(x, w, b, s, lens)
    chk(rc)
    with mode("bf16"), launched("hfg_tconv_kernel/bf16"):
        assert lib().fcl_get_gemm_mode() == _lib.GEMM_BF16
        rc, y1, yp1 = run_tconv(x, w, b, s, lens)
        chk(rc)
    assert lib().fcl_get_gemm_mode() == _lib.GEMM_F32
    scale = max(1.0, float(np.abs(ref).max()))
    g0, g1 = y0.t.cpu().numpy().reshape(ref.shape), y1.t.cpu().numpy().reshape(ref.shape)
    print("bf16 tconv: err %.3e bound %.3e, away from default %.3e" % (max_abs(g1, ref), BF16_GEMM * scale, max_abs(g1, g0)))
    assert max_abs(g1, ref) <= BF16_GEMM * scale and max_abs(g1, g0) > 1e-4 * scale
    assert np.array_equal(planes_of(yp1, ref.shape[0]), split_planes_np(lrelu32(g1, SLOPE)))  # outputs keep both planes
    # single convolution
    lens = [20, 1, 100, 7, 130]
    rng = np.random.RandomState(R.SEEDS["bf16"])
    xc = rng.standard_normal((sum(lens), 80)).astype(np.float32)
    wc, bc = (rng.standard_normal((128, 80, 7)) / np.sqrt(560)).astype(np.float32), (0.5 * rng.standard_normal(128)).astype(np.float32)
    ref = torch.cat(per_utt(lambda xs: R.conv1d(rb(R.f64(xs)), R.f64(wc), R.f64(bc), 1, rb), xc, lens)).numpy()
    y0, _ = run_conv(xc, wc, bc, 1, lens)
    with mode("bf16"), launched("hfg_conv_kernel/bf16"):
        y1, _ = run_conv(xc, wc, bc, 1, lens)
    scale = max(1.0, float(np.abs(ref).max()))
    g0, g1 = y0.t.cpu().numpy().reshape(ref.shape), y1.t.cpu().numpy().reshape(ref.shape)
    print("bf16 conv: err %.3e bound %.3e, away from default %.3e" % (max_abs(g1, ref), BF16_GEMM * scale, max_abs(g1, g0)))
    assert max_abs(g1, ref) <= BF16_GEMM * scale and max_abs(g1, g0) > 1e-4 * scale
    # residual unit: fused (64, 128) and one launch per convolution (256)
    for kr, dil, c in ((7, 3, 64), (11, 5, 128), (3, 1, 256)):
        case = R.unit_case(R.SEEDS["bf16"], kr, dil, c, lens)
        x, w1, b1, w2, b2, _ = case
        m = x.shape[0]
        xt_ref = torch.cat(per_utt(lambda xs: R.conv1d(rb(R.lrelu(R.f64(xs), SLOPE)), R.f64(w1), R.f64(b1), dil, rb), x, lens))
        with mode("bf16"), launched("hfg_conv_kernel/bf16"):
            y1, yp1 = run_conv(lrelu32(x, SLOPE), w1, b1, dil, lens)
        xt = y1.t.cpu().numpy().reshape(m, c)
        s1 = max(1.0, float(xt_ref.abs().max()))
        e1 = max_abs(xt, xt_ref.numpy())
        assert e1 <= BF16_GEMM * s1, (kr, dil, c, e1)
        hi = bf16_to_f32(planes_of(yp1, m)[:, :, 0, :]).reshape(m, c)  # the bf16 operand conv2 reads, as the kernel wrote it
        assert np.array_equal(hi, bf16_to_f32(split_planes_np(lrelu32(xt, SLOPE))[:, :, 0, :]).reshape(m, c))
        conv2_ref = torch.cat(per_utt(lambda hs: R.conv1d(R.f64(hs), R.f64(w2), R.f64(b2), 1, rb), hi, lens))
        with mode("bf16"), launched("hfg_conv_kernel/bf16"):
            y2, _ = run_conv(hi, w2, b2, 1, lens, resid=x)
        two = y2.t.cpu().numpy().reshape(m, c)
        s2 = max(1.0, float(conv2_ref.abs().max()))
        want = conv2_ref.numpy() + x.astype(np.float64)
        e2 = max_abs(two, want)
        assert e2 <= BF16_GEMM * s2 + 2.0 ** -23 * float(np.abs(want).max()), (kr, dil, c, e2)
        g0 = run_unit(case, kr, dil, lens, "mid")["x"].t.cpu().numpy().reshape(m, c)
        with mode("bf16") as sfx:
            out = run_unit(case, kr, dil, lens, "acc", sfx)
        g1 = out["x"].t.cpu().numpy().reshape(m, c)
        e3 = max_abs(g1, two)
        print("bf16 unit kr=%d d=%d C=%d: conv1 %.3e (bound %.3e), conv2 on the written bf16 values %.3e (bound %.3e), unit kernel - two launches %.3e, "
              "away from default %.3e" % (kr, dil, c, e1, BF16_GEMM * s1, e2, BF16_GEMM * s2, e3, max_abs(g1, g0)))
        assert e3 <= BF16_GEMM * s2 and max_abs(g1, g0) > 1e-4 * s2
        check_unit_outputs(out, g1, case, "acc", BF16_GEMM * s2, lens)
    # output stage: hi plane of the operand, bf16-rounded weights
    rng = np.random.RandomState(R.SEEDS["bf16"] + 1)
    lens = [1, 2, 40, 3, 300]
    a32 = lrelu32(rng.standard_normal((sum(lens), 32)).astype(np.float32), R.OUT_SLOPE)
    w, b = (rng.standard_normal((1, 32, 7)) / np.sqrt(224)).astype(np.float32), (0.5 * rng.standard_normal(1)).astype(np.float32)
    pre = torch.cat(per_utt(lambda xs: R.conv1d(rb(xs), R.f64(w), R.f64(b), 1, rb), R.f64(a32), lens))
    w0 = run_out(a32, w, b, lens).t.cpu().numpy()
    with mode("bf16"), launched("hfg_out_kernel/bf16"):
        w1 = run_out(a32, w, b, lens).t.cpu().numpy()
    scale = max(1.0, float(pre.abs().max()))
    e = max_abs(w1.reshape(-1, 1), torch.tanh(pre).numpy())
    print("bf16 output conv: err %.3e bound %.3e, away from default %.3e" % (e, BF16_GEMM * scale, max_abs(w1, w0)))
    assert e <= BF16_GEMM * scale and max_abs(w1, w0) > 1e-4 * scale


# ------------------------------------------------------------------------------------------------------------------ 7 refusals
def test_refused_geometries(hfg):
    from fcl_taco2_amd import _lib

    x, w, b = R.tconv_case(1, 4, 64, [5])
    rc, y, yp = run_tconv(x, w[:, :, :6], b, 4, [5], ksize=6)  # ku % s != 0
    assert rc == -2 and b"multiple of the stride" in lib().fcl_last_error()
    rc, y, yp = run_tconv(x, np.concatenate([w, w], axis=2), b, 4, [5])  # ku = 4 s: not s x the input rows with the package's padding
    assert rc == -2 and b"padding" in lib().fcl_last_error()
    assert bool((y.bits() == PAT32).all()) and bool((yp.bits() == PAT16).all())
    u = _lib.HfgUnit()
    u.m, u.c, u.ksize, u.dilation, u.rate = 10, 48, 3, 1, 1
    buf, buf2 = torch.zeros(1 << 20, dtype=torch.int32, device=DEV), torch.zeros(1 << 20, dtype=torch.int32, device=DEV)  # real memory, larger than
    for f in ("xp", "x", "w1p", "b1", "w2p", "b2", "frame_utt", "utt_off", "x_out"):                                       # anything these shapes touch
        setattr(u, f, buf.data_ptr())
    u.xp_out = buf2.data_ptr()
    assert lib().fcl_hfg_unit_fwd(C.byref(u), None) == -2 and b"multiple of 32" in lib().fcl_last_error()
    u.c, u.ksize = 64, 9
    assert lib().fcl_hfg_unit_fwd(C.byref(u), None) == -2 and b"kernel size" in lib().fcl_last_error()
    u.ksize, u.c = 3, 256
    assert lib().fcl_hfg_unit_fwd(C.byref(u), None) == -5 and b"workspace tp" in lib().fcl_last_error()
    with pytest.raises(NotImplementedError, match="upsample_kernel_sizes"):
        hfg.config(dict(upsample_kernel_sizes=(16, 12, 4, 4)))
    with pytest.raises(_lib.FclError, match="no capacity form"):
        from fcl_taco2_amd import engine

        class _Plan(object):
            class hp(object):
                odim = 80
            device = DEV

        class _Gen(object):
            class plan(object):
                A, device, eager_only, hop = 80, DEV, True, 256

        engine.SpeechRunner(_Plan(), _Gen(), 1, 8, None)


def test_exact_fp32_mode_refuses_in_a_child_process(hfg):
    code = """
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import ctypes as C
import numpy as np
import fcl_taco2_amd
from fcl_taco2_amd import _lib, hifigan
import hifigan_ref as R
import torch
lib = _lib.load()
buf = torch.zeros(1 << 20, dtype=torch.int32, device="cuda:0")  # real memory, larger than anything these shapes touch
P = buf.data_ptr()
def fill(a, names):
    for n in names:
        setattr(a, n, P)
    return a
t = fill(_lib.HfgTconv(), ("xp", "wp", "bias", "frame_utt", "utt_off", "y"))
t.m_in, t.cin, t.cout, t.stride, t.ksize, t.padding, t.rate_in = 4, 64, 32, 2, 4, 1, 1
u = fill(_lib.HfgUnit(), ("xp", "x", "w1p", "b1", "w2p", "b2", "frame_utt", "utt_off", "x_out"))
u.m, u.c, u.ksize, u.dilation, u.rate = 4, 64, 3, 1, 1
c = fill(_lib.HfgConv(), ("xp", "wp", "bias", "frame_utt", "utt_off", "y"))
c.m, c.cin, c.cout, c.ksize, c.dilation, c.rate = 4, 64, 32, 3, 1, 1
for rc in (lib.fcl_hfg_tconv_fwd(C.byref(t), None), lib.fcl_hfg_unit_fwd(C.byref(u), None), lib.fcl_hfg_conv_fwd(C.byref(c), None),
           lib.fcl_hfg_out_fwd(P, P, P, P, P, 1, P, 4, 32, 1, 7, None)):
    assert rc == -1 and b"FCL_PRECISION=0" in lib.fcl_last_error(), (rc, lib.fcl_last_error())
try:
    hifigan.HiFiGANPlan(R.random_state_dict(np.random.RandomState(0), R.SMALL), "cuda:0", R.plan_cfg(R.SMALL))
except _lib.FclError as e:
    assert "FCL_PRECISION=0" in str(e)
else:
    raise SystemExit("HiFiGANPlan did not refuse")
print("REFUSED")
""" % (ROOT, os.path.join(ROOT, "tests"))
    env = dict(os.environ, FCL_PRECISION="0")
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "REFUSED" in p.stdout, (p.stdout[-2000:], p.stderr[-2000:])


# ------------------------------------------------------------------------------------------------------------------ 8 drivers
HFG_YML = """sampling_rate: 24000
generator_type: HiFiGANGenerator
generator_params:
  channels: 128
  upsample_scales: [4, 2]
  upsample_kernel_sizes: [8, 4]
  nonlinear_activation_params: {negative_slope: 0.1}
"""


def _read_wav(path):
    with wave.open(str(path)) as f:
        return (f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()), np.frombuffer(f.readframes(f.getnframes()), dtype="<i2")


def _checkpoint(tmp_path):
    sd = R.random_state_dict(np.random.RandomState(R.SEEDS["drivers"]), R.SMALL)
    stored = R.with_weight_norm(sd, np.random.RandomState(R.SEEDS["drivers"] + 1))  # as the package stores it: weight_g / weight_v
    torch.save({"model": {"generator": {k: torch.from_numpy(v) for k, v in stored.items()}}}, tmp_path / "hifigan.pkl")
    (tmp_path / "config.yml").write_text(HFG_YML)
    return sd


def test_vocoder_decode_on_a_hifigan_checkpoint(hfg, tmp_path):
    from fcl_taco2_amd import vocoder, vocoder_decode as V

    _checkpoint(tmp_path)
    gen, rate = V.build_generator(str(tmp_path / "hifigan.pkl"), DEV)
    assert isinstance(gen, hfg.HiFiGANGenerator) and rate == 24000 and gen.plan.hop == 8
    rng = np.random.RandomState(4)
    feats = [("utt%d" % i, rng.standard_normal((n, 80)).astype(np.float32)) for i, n in enumerate([30, 1, 17, 50, 2])]
    with launched("hfg_unit_kernel<32>", "hfg_unit_kernel<64>", "hfg_tconv_kernel", "hfg_out_kernel"):
        samples, _ = V.decode(gen, feats, str(tmp_path / "wav"), rate, batch_frames=40)  # several batches
    assert samples == 8 * sum(m.shape[0] for _, m in feats)
    for uid, m in feats:
        hdr, pcm = _read_wav(tmp_path / "wav" / (uid + "_gen.wav"))
        want = vocoder.pcm16(gen.synthesize([m])[0])
        assert hdr == (1, 2, 24000, 8 * m.shape[0]) and np.array_equal(pcm, want) and np.abs(pcm).max() > 0, uid
    # without the config.yml the family comes from the state-dict keys and the geometry from the shapes
    os.remove(tmp_path / "config.yml")
    gen2, rate2 = V.build_generator(str(tmp_path / "hifigan.pkl"), DEV)
    assert isinstance(gen2, hfg.HiFiGANGenerator) and rate2 == 22050
    assert torch.equal(gen2.synthesize([feats[0][1]])[0], gen.synthesize([feats[0][1]])[0])


def test_tts_driver_with_a_hifigan_generator(hfg, tmp_path):
    """text -> waveform with a generator that has no capacity form: every batch takes the two-step route and is counted as eager"""
    from fcl_taco2_amd import hparams as HP, synthetic as SYN, tts as TTS, vocoder
    from fcl_taco2_amd.kaldi_io import read_scp

    _checkpoint(tmp_path)
    hp = HP.student_hparams(dropout_rate=0.0)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in SYN.closed_form_state_dict(HP.param_spec(hp, HP.teacher_hparams(), True)).items()}
    sd["duration_predictor.linear.weight"] = torch.zeros_like(sd["duration_predictor.linear.weight"])
    sd["duration_predictor.linear.bias"] = torch.full((1,), float(np.log(4.0)))  # every phoneme predicts 3 frames
    torch.save({"model": sd, "optimizer": {}}, tmp_path / "snapshot.ep.1")
    args = dict(model_module="nets.knowledge_distillation.e2e_tts_tacotron2_sa_kd_student:Tacotron2_sa", embed_dim=256, eunits=256,
                econv_chans=256, dunits=256, postnet_chans=128, use_residual=False, use_masking=True, dropout_rate=0.0, share_proj=True)
    (tmp_path / "model.json").write_text(json.dumps([80, 80, args]))
    (tmp_path / "teacher.json").write_text(json.dumps([80, 80, dict(use_residual=False)]))
    rng = np.random.RandomState(3)
    utts = {"u%02d" % i: {"output": [{"tokenid": " ".join(map(str, rng.randint(1, 80, size=rng.randint(5, 40))))}]} for i in range(7)}
    (tmp_path / "data.json").write_text(json.dumps({"utts": utts}))
    lens = {k: len(v["output"][0]["tokenid"].split()) for k, v in utts.items()}
    with launched("hfg_unit_kernel<32>", "hfg_unit_kernel<64>", "hfg_tconv_kernel", "hfg_out_kernel"):
        res = TTS.main(["--model", str(tmp_path / "snapshot.ep.1"), "--model-conf", str(tmp_path / "model.json"), "--teacher-config", str(tmp_path / "teacher.json"),
                        "--json", str(tmp_path / "data.json"), "--vocoder-checkpoint", str(tmp_path / "hifigan.pkl"), "--batch-size", "3", "--verbose", "0",
                        "--seed", "11", "--outdir", str(tmp_path / "wav"), "--feats-out", str(tmp_path / "feats")])
    assert res["eager_batches"] == 3 == len(res["batches"]) and res["graph_batches"] == 0 and res["redone_batches"] == 0
    assert res["samples"] == 8 * 3 * sum(lens.values())
    mels = read_scp(str(tmp_path / "feats.scp"))
    from fcl_taco2_amd import vocoder_decode as V

    gen, _ = V.build_generator(str(tmp_path / "hifigan.pkl"), DEV)
    for route, ids, _seed in res["batches"]:
        rows = torch.from_numpy(np.concatenate([mels[k] for k in ids])).to(DEV)
        want = gen.synthesize_packed(rows, [mels[k].shape[0] for k in ids])
        for k, w in zip(ids, want):
            hdr, pcm = _read_wav(tmp_path / "wav" / (k + "_gen.wav"))
            assert hdr == (1, 2, 24000, 8 * 3 * lens[k]) and np.array_equal(pcm, vocoder.pcm16_rule(w.cpu().numpy())), (route, k)
