"""-m gpu: every kernel of the Parallel WaveGAN stage (csrc/pwg.hip, the one-launch blocks and the fused last stage of csrc/gemm_planes.hip) on its
own against a float64 statement of the same operation (helpers.py: plain numpy / torch, one utterance at a time, so utterance edges are real zero
padding), on random inputs that saturate the gate (tests/test_vocoder_inputs_cpu.py asserts that they do).  Every buffer a kernel writes carries
guard lines in front and behind, filled with a NaN bit pattern, and they must survive.  Bounds are computed from the float64 reference and the
project's bound for the pre-split GEMM (3e-5 at unit scale, test_gpu_planes.py); DESIGN.md 6b lists which test pins which kernel variant.

  1 fcl_pwg_upsample_stage      2 fcl_pwg_aux_coeff      3 fcl_pwg_first_conv / fcl_pwg_last_fwd
  4 one residual block per call of fcl_pwg_layer_fwd / fcl_pwg_layer_cap_fwd, teacher-forced, every kernel variant
  5 the whole generator on random weights, all 30 taps against float64
  6 the FCL_GEMM_BF16 form of every vocoder kernel"""
import contextlib
import ctypes as C
import math

import numpy as np
import pytest
import torch

import helpers as H
from helpers import bf16_rn, bf16_to_f32, max_abs, split_planes_np

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAT16, PAT32 = 0x7FC1, 0x7FC12345  # a bf16 / an fp32 NaN: whatever is read from an unwritten or dead line poisons the result
SQH = math.sqrt(0.5)


@pytest.fixture(scope="module")
def voc():
    assert torch.cuda.is_available()
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib, ops, vocoder

    _lib.load()
    if not ops.planes_enabled():
        pytest.skip("FCL_PRECISION=0 / FCL_PLANES=0: the vocoder needs the pre-split operand path")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    return vocoder


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

    PAD = 8192  # elements; a multiple of 128 bytes for both element types

    def __init__(self, n, dtype):
        self.n, self.dtype = int(n), dtype
        self.buf = torch.empty(self.n + 2 * self.PAD, dtype=dtype, device=DEV)
        self.bits().fill_(self.pattern())
        assert self.t.data_ptr() % 128 == 0

    def pattern(self):
        return PAT16 if self.dtype == torch.int16 else PAT32

    def bits(self):
        return self.buf if self.dtype == torch.int16 else self.buf.view(torch.int32)

    @property
    def t(self):
        return self.buf[self.PAD : self.PAD + self.n]

    def intact(self):
        b, p = self.bits(), self.pattern()
        return bool((b[: self.PAD] == p).all()) and bool((b[self.PAD + self.n :] == p).all())

    def untouched(self, view):
        """`view` (a slice of the payload) still holds the pattern"""
        v = view if self.dtype == torch.int16 else view.view(torch.int32)
        return bool((v == self.pattern()).all())


def planes_np(t, rows):
    """device planes, row-major [rows, L * 64] -> uint16 [rows, L, 2, 32]"""
    return t.cpu().numpy().view(np.uint16).reshape(rows, -1, 2, 32)


def planes_value(raw):
    """uint16 [..., 2, 32] -> float64 hi + lo [..., 32]"""
    return bf16_to_f32(raw[..., 0, :]).astype(np.float64) + bf16_to_f32(raw[..., 1, :]).astype(np.float64)


def chunk_major(p, rows):
    """row-major planes [rows, L * 64] -> chunk-major [L, rows, 64]"""
    return p.reshape(rows, -1, 64).permute(1, 0, 2).contiguous()


def f64(a):
    return torch.from_numpy(np.asarray(a)).to(torch.float64)


# ------------------------------------------------------------------------------------------------------------------ 1 upsample stage
@pytest.mark.parametrize("scale", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("rate_in", [1, 4, 64])
@pytest.mark.parametrize("c", [4, 8, 20, 80, 100])
def test_upsample_stage_vs_float64(voc, scale, rate_in, c):
    """nearest stretch + zero-padded 1 x (2s+1) convolution per utterance; fp32 within (2s+2) * 2^-24 * max sum|w||x| (2s additions of the taps that
    collapse onto one input row, 3 FMAs); planes = the documented split of the fp32 result, bit for bit, zero past C in both planes"""
    rng = np.random.RandomState(scale * 1000 + rate_in * 10 + c)
    for lens in ([1], [1, 1, 1], [3, 1, 7, 2]):
        frames = sum(lens)
        rows_in, rows_out = frames * rate_in, frames * rate_in * scale
        x = rng.standard_normal((rows_in, c)).astype(np.float32)
        w = rng.standard_normal(2 * scale + 1).astype(np.float32)
        ref, mag, r0 = [], [], 0
        for n in lens:
            xs = f64(x[r0 : r0 + n * rate_in])
            ref.append(H.pwg_stage_f64(xs, scale, f64(w)))
            mag.append(H.pwg_stage_f64(xs.abs(), scale, f64(w).abs()))
            r0 += n * rate_in
        ref, mag = torch.cat(ref).numpy(), torch.cat(mag).numpy()
        tol = (2 * scale + 2) * 2.0 ** -24 * float(mag.max())
        fu = dev(np.repeat(np.arange(len(lens)), lens).astype(np.int32))
        uo = dev(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32))
        xd, wd = dev(x), dev(w)
        ldp = (c + 31) // 32
        out = Guarded(rows_out * c, torch.float32)
        chk(lib().fcl_pwg_upsample_stage(xd.data_ptr(), fu.data_ptr(), uo.data_ptr(), frames, rate_in, scale, wd.data_ptr(), out.t.data_ptr(), None, c, 0, stream()))
        got = out.t.reshape(rows_out, c).cpu().numpy()
        err = max_abs(got, ref)
        assert err <= tol, (lens, err, tol)
        assert out.intact()
        want_p = split_planes_np(got)
        for cm in (0, 1):
            op = Guarded(rows_out * ldp * 64, torch.int16)
            chk(lib().fcl_pwg_upsample_stage(xd.data_ptr(), fu.data_ptr(), uo.data_ptr(), frames, rate_in, scale, wd.data_ptr(), None, op.t.data_ptr(), c, cm, stream()))
            raw = op.t.cpu().numpy().view(np.uint16)
            raw = raw.reshape(ldp, rows_out, 2, 32).transpose(1, 0, 2, 3) if cm else raw.reshape(rows_out, ldp, 2, 32)
            assert np.array_equal(raw, want_p), (lens, cm)
            assert not raw.transpose(0, 2, 1, 3).reshape(rows_out, 2, ldp * 32)[:, :, c:].any()
            assert op.intact()
        both_f, both_p = Guarded(rows_out * c, torch.float32), Guarded(rows_out * ldp * 64, torch.int16)  # both outputs of one launch
        chk(lib().fcl_pwg_upsample_stage(xd.data_ptr(), fu.data_ptr(), uo.data_ptr(), frames, rate_in, scale, wd.data_ptr(), both_f.t.data_ptr(),
                                         both_p.t.data_ptr(), c, 0, stream()))
        assert torch.equal(both_f.t, out.t) and np.array_equal(both_p.t.cpu().numpy().view(np.uint16).reshape(rows_out, ldp, 2, 32), want_p)
        assert both_f.intact() and both_p.intact()


# ------------------------------------------------------------------------------------------------------------------ 2 coefficient lines
def aux_coeff_rule(kc, hop, frames):
    """numpy statement of fcl_pwg_aux_coeff (include/fcl_hip.h): uint16 [M, 2, 32]"""
    m = np.arange(kc.shape[0])
    f = m // hop
    r = f & 31
    w0 = np.where((r >= 2) & (r <= 29), (f >> 5) * 32, ((f + 16) >> 5) * 32 - 16)
    out = np.zeros((kc.shape[0], 2, 32), np.uint16)
    for d in range(5):
        g = f - 2 + d
        ok = (g >= 0) & (g < frames)
        v = kc[m, g % 5].astype(np.float32)
        hi = bf16_rn(v)
        lo = bf16_rn(v - bf16_to_f32(hi))
        col = g - w0
        assert not ok.any() or (col[ok].min() >= 0 and col[ok].max() < 32)
        out[m[ok], 0, col[ok]] = hi[ok]
        out[m[ok], 1, col[ok]] = lo[ok]
    return out


@pytest.mark.parametrize("frames", [1, 2, 3, 31, 32, 33, 70])
@pytest.mark.parametrize("hop", [128, 256, 384])
def test_aux_coeff_lines_bit_for_bit(voc, frames, hop):
    rng = np.random.RandomState(frames * 7 + hop)
    M = frames * hop
    kc = rng.standard_normal((M, 8)).astype(np.float32)
    kp = Guarded(M * 64, torch.int16)
    kcd = dev(kc)
    chk(lib().fcl_pwg_aux_coeff(kcd.data_ptr(), M, hop, frames, kp.t.data_ptr(), stream()))
    got = kp.t.cpu().numpy().view(np.uint16).reshape(M, 2, 32)
    assert np.array_equal(got, aux_coeff_rule(kc, hop, frames))
    assert kp.intact()


# ------------------------------------------------------------------------------------------------------------------ 3 first / last stage
@pytest.mark.parametrize("r", [32, 64, 96])
@pytest.mark.parametrize("m", [1, 127, 128, 129, 1000])
def test_first_conv_vs_float64(voc, r, m):
    rng = np.random.RandomState(r + m)
    z, w, b = (rng.standard_normal(n).astype(np.float32) for n in (m, r, r))
    ref = z.astype(np.float64)[:, None] * w.astype(np.float64)[None, :] + b.astype(np.float64)
    tol = 2.0 ** -23 * float((np.abs(z)[:, None] * np.abs(w)[None, :] + np.abs(b)).max())  # one product, one sum (or one FMA)
    zd, wd, bd = dev(z), dev(w), dev(b)
    first = None
    for cm in (0, 1):
        x, xp = Guarded(m * r, torch.float32), Guarded(m * r * 2, torch.int16)
        chk(lib().fcl_pwg_first_conv(zd.data_ptr(), wd.data_ptr(), bd.data_ptr(), x.t.data_ptr(), xp.t.data_ptr(), m, r, cm, stream()))
        got = x.t.reshape(m, r).cpu().numpy()
        assert max_abs(got, ref) <= tol
        raw = xp.t.cpu().numpy().view(np.uint16)
        raw = raw.reshape(r // 32, m, 2, 32).transpose(1, 0, 2, 3) if cm else raw.reshape(m, r // 32, 2, 32)
        assert np.array_equal(raw, split_planes_np(got))
        assert x.intact() and xp.intact()
        first = got if first is None else first
        assert np.array_equal(got, first)
        xp2 = Guarded(m * r * 2, torch.int16)  # planes only (the one-launch blocks' form)
        chk(lib().fcl_pwg_first_conv(zd.data_ptr(), wd.data_ptr(), bd.data_ptr(), None, xp2.t.data_ptr(), m, r, cm, stream()))
        assert torch.equal(xp2.t, xp.t) and xp2.intact()


def last_stage_inputs(s, m, seed):
    """skips of both signs at a scale where both ReLUs cut about half of the channels"""
    rng = np.random.RandomState(seed)
    sk = (6.0 * rng.standard_normal((m, s))).astype(np.float32)
    w1 = (rng.standard_normal((s, s)) / math.sqrt(s)).astype(np.float32)
    b1, w2 = (0.1 * rng.standard_normal(s)).astype(np.float32), (rng.standard_normal(s) / math.sqrt(s)).astype(np.float32)
    return sk, w1, b1, w2, 0.25, math.sqrt(1.0 / 30)


def last_stage_ref(sk, w1, b1, w2, b2, scale, rnd=None):
    r = rnd or (lambda t: t)
    y = torch.relu(f64(sk) * scale)
    h = r(y) @ r(f64(w1)).t() + f64(b1)
    wav = torch.relu(h) @ f64(w2) + b2
    return y, h, wav


def last_stage_tol(h, w2, gemm=3e-5):
    """GEMM bound on h; ReLU is 1-Lipschitz; the 64 -> 1 projection adds S fp32 roundings of its partial sums"""
    tol_h = gemm * max(1.0, float(h.abs().max()))
    dot = float((torch.relu(h) * f64(w2).abs()).sum(1).max())
    return tol_h * float(np.abs(w2).sum()) + (len(w2) + 2) * 2.0 ** -24 * max(dot, 1.0)


@pytest.mark.parametrize("s", [64, 32, 96])
@pytest.mark.parametrize("m", [1, 127, 128, 129, 1000])
def test_last_stage_vs_float64(voc, s, m):
    """S = 64: the one-launch kernel (pwg_last_kernel); 32 / 96: ReLU * scale -> planes, the GEMM, the output kernel"""
    from fcl_taco2_amd import ops

    sk, w1, b1, w2, b2, scale = last_stage_inputs(s, m, s * 13 + m)
    y, h, ref = last_stage_ref(sk, w1, b1, w2, b2, scale)
    assert 0.3 < float((y > 0).double().mean()) < 0.7 and 0.3 < float((h > 0).double().mean()) < 0.7
    skd, w1p, b1d, w2d = dev(sk), ops.pack_planes(dev(w1)), dev(b1), dev(w2)
    wav = Guarded(m, torch.float32)
    yp, hb = Guarded(m * s * 2, torch.int16), Guarded(m * s, torch.float32)
    with launched("pwg_last_kernel") if s == 64 else contextlib.nullcontext():
        chk(lib().fcl_pwg_last_fwd(skd.data_ptr(), scale, w1p.data_ptr(), b1d.data_ptr(), w2d.data_ptr(), b2, None if s == 64 else yp.t.data_ptr(),
                                   None if s == 64 else hb.t.data_ptr(), wav.t.data_ptr(), m, s, stream()))
    err, tol = max_abs(wav.t.cpu().numpy(), ref.numpy()), last_stage_tol(h, w2)
    print("last stage S=%d M=%d: err %.3g tol %.3g" % (s, m, err, tol))
    assert err <= tol
    assert wav.intact() and yp.intact() and hb.intact()
    assert torch.equal(skd.cpu(), torch.from_numpy(sk))
    if s != 64:  # the general path's workspaces: ReLU(skips * scale) as planes, bit for bit, and the GEMM result
        y32 = np.maximum(sk * np.float32(scale), np.float32(0))
        assert np.array_equal(planes_np(yp.t.reshape(m, -1), m), split_planes_np(y32))
        assert max_abs(hb.t.reshape(m, s).cpu().numpy(), h.numpy()) <= 3e-5 * max(1.0, float(h.abs().max()))


# ------------------------------------------------------------------------------------------------------------------ 4 one block per call
class Block(object):
    """One residual block's device operands, filled the way synthesize_packed fills fcl_pwg_layer_t, with guarded outputs.  mode: 'unfused'
    (four launches, row-major planes), 'fused' (one launch, chunk-major planes); features either given (`feats`) or at frame rate (`mels`, one per
    utterance, whole frames); cap: capacity in samples (the rows past the live ones are dead: NaN planes, NaN skips, NaN features)."""

    def __init__(self, voc, plan, sd, cfg, seed):
        self.voc, self.plan, self.sd, self.cfg = voc, plan, sd, cfg
        self.w = H.pwg_layer_weights_f64(sd, 0)
        self.gen = voc.ParallelWaveGANGenerator(plan)
        self.seed = seed

    def run(self, x, skips0, lens, d, first, fused, feats=None, mels=None, cap=0):
        from fcl_taco2_amd import _lib, ops

        pl = self.plan
        R, A, k, L = pl.R, pl.A, pl.k, pl.layers[0]
        nl, ldc = R // 32, (A + 31) // 32
        M = int(sum(lens)) * (pl.hop if mels is not None else 1)
        Mc = cap or M
        rows = [n * (pl.hop if mels is not None else 1) for n in lens] + ([Mc - M] if Mc > M else [])
        lo, hi = H.seg_bounds(rows)
        seg_lo, seg_hi = dev(lo), dev(hi)
        xp_rm = ops.pack_planes(dev(x))
        a = _lib.PwgLayer()
        a.m, a.r, a.aux, a.ksize, a.dilation, a.first_layer = Mc, R, A, k, d, int(first)
        a.seg_lo, a.seg_hi = seg_lo.data_ptr(), seg_hi.data_ptr()
        a.w_conv_p, a.b_conv, a.w_aux_p = L["w_conv_p"].data_ptr(), L["b_conv"].data_ptr(), L["w_aux_p"].data_ptr()
        a.w_os_p, a.b_os = L["w_os_p"].data_ptr(), L["b_os"].data_ptr()
        skips = Guarded(Mc * R, torch.float32)
        if not first:
            skips.t[: M * R] = dev(skips0).reshape(-1)
        a.skips = skips.t.data_ptr()
        keep = [seg_lo, seg_hi, xp_rm]
        if fused:
            xin, xout = Guarded(nl * Mc * 64, torch.int16), Guarded(nl * Mc * 64, torch.int16)
            xin.t.reshape(nl, Mc, 64)[:, :M] = chunk_major(xp_rm, M)
            before = xin.buf.clone()
            a.x, a.xp, a.xp_out = None, xin.t.data_ptr(), xout.t.data_ptr()
            if mels is not None:
                frames_all = list(lens) + ([(Mc - M) // pl.hop] if Mc > M else [])
                rng = np.random.RandomState(self.seed + 77)
                mel_rows = np.concatenate(list(mels) + ([2.5 * rng.standard_normal((frames_all[-1], A)).astype(np.float32)] if Mc > M else []))
                kp, pt_a, pt_b, ld_pt = self.gen._aux_frame_rate(dev(mel_rows.astype(np.float32)), self.gen._maps(frames_all))
                a.kp, a.pt_a, a.pt_b, a.ld_pt, a.hop = kp.data_ptr(), pt_a.data_ptr(), pt_b.data_ptr(), ld_pt, pl.hop
                keep += [kp, pt_a, pt_b]
                self.fr = (kp, pt_a, pt_b, ld_pt)
            else:
                cp = torch.full((ldc, Mc, 64), PAT16, dtype=torch.int16, device=DEV)
                cp[:, :M] = chunk_major(ops.pack_planes(dev(feats)), M)
                assert cp.data_ptr() % 128 == 0
                a.cp = cp.data_ptr()
                keep.append(cp)
            if cap:
                live = dev(np.array([M // max(pl.hop, 1), M, 0, len(lens)], dtype=np.int32))
                chk(lib().fcl_pwg_layer_cap_fwd(C.byref(a), live.data_ptr(), stream()))
            else:
                chk(lib().fcl_pwg_layer_fwd(C.byref(a), stream()))
            torch.cuda.synchronize()
            assert torch.equal(xin.buf, before)  # x is read, never written (neighbouring tiles still need it)
            out3 = xout.t.reshape(nl, Mc, 64)
            x_out = planes_value(out3[:, :M].permute(1, 0, 2).contiguous().cpu().numpy().view(np.uint16).reshape(M, nl, 2, 32)).reshape(M, R)
            assert xout.intact() and xout.untouched(out3[:, M:])  # nothing past M in either chunk, nothing in the dead samples
        else:
            xf, xp = Guarded(M * R, torch.float32), Guarded(M * nl * 64, torch.int16)
            xf.t[:] = dev(x).reshape(-1)
            xp.t[:] = xp_rm.reshape(-1)
            zb, ob, gp = Guarded(M * 2 * R, torch.float32), Guarded(M * 2 * R, torch.float32), Guarded(M * nl * 64, torch.int16)
            cp = ops.pack_planes(dev(feats))
            a.x, a.xp, a.cp, a.z, a.gp, a.o = xf.t.data_ptr(), xp.t.data_ptr(), cp.data_ptr(), zb.t.data_ptr(), gp.t.data_ptr(), ob.t.data_ptr()
            keep.append(cp)
            chk(lib().fcl_pwg_layer_fwd(C.byref(a), stream()))
            torch.cuda.synchronize()
            x32 = xf.t.reshape(M, R).cpu().numpy()
            # the planes carry the fp32 result: hi word bit for bit, hi + lo to the format's 2^-15 (pwg_resid_kernel's lo word is not always the
            # split of the STORED fp32 value in its last bit -- DESIGN.md 6b -- so the value is compared, and both forms go against the reference)
            raw = planes_np(xp.t.reshape(M, nl * 64), M)
            assert np.array_equal(raw[:, :, 0], split_planes_np(x32)[:, :, 0])
            pv = planes_value(raw).reshape(M, R)
            assert np.all(np.abs(pv - x32) <= 2.0 ** -15 * np.abs(x32))
            x_out, self.x_f32 = pv, x32.astype(np.float64)
            assert all(g.intact() for g in (xf, xp, zb, ob, gp))
        assert skips.intact() and skips.untouched(skips.t[M * R :])
        return x_out, skips.t[: M * R].reshape(M, R).cpu().numpy().astype(np.float64)

    def reference(self, x, skips0, rows, d, first, aux_terms, rnd=None, rnd_g=None):
        """float64 block per utterance; x enters as the value its planes carry.  Returns x_out, skips and the bounds of the module docstring."""
        xv = H.plane_round(f64(x))
        x_op = xv if rnd is None else rnd(f64(x))  # a rounded mode reads the hi plane = the rounding of the fp32 value itself
        xs, ss, zmax, omax, r0 = [], [], 0.0, 0.0, 0
        for n, at in zip(rows, aux_terms):
            o = H.pwg_block_f64(xv[r0 : r0 + n], at, self.w, d, rnd, rnd_g, x_op=x_op[r0 : r0 + n])
            xs.append(o["x_out"])
            ss.append(o["skip"])
            zmax = max(zmax, float(o["z"].abs().max()))
            omax = max(omax, float((o["x_out"] / SQH - xv[r0 : r0 + n]).abs().max()), float(o["skip"].abs().max()))
            r0 += n
        x_ref, s_ref = torch.cat(xs), torch.cat(ss)
        if not first:
            s_ref = s_ref + f64(skips0)
        return x_ref, s_ref, zmax, omax

    def bounds(self, x_ref, zmax, omax, gemm=3e-5):
        w_os_l1 = float(torch.cat([self.w["out"], self.w["skip"]]).abs().sum(1).max())
        tol_z = gemm * max(1.0, zmax)
        tol_o = 2 * tol_z * w_os_l1 + gemm * max(1.0, omax)  # the gate is 1-Lipschitz in each of its two arguments
        return tol_o * SQH + 2.0 ** -15 * float(x_ref.abs().max()), tol_o


def make_block(voc, r, aux, ksize=3, scales=(2,), seed=0):
    sd, cfg = H.pwg_block_state_dict(seed, r, aux, ksize, scales)
    return Block(voc, voc.PWGPlan(sd, DEV, cfg), sd, cfg, seed)


def sweep_features_given(blk, fused, kernel):
    """lens x dilations x first_layer with the features given as a random [M, aux] array; returns the worst err / bound ratios"""
    R, A = blk.plan.R, blk.plan.A
    worst = [0.0, 0.0]
    probe = True
    for m, lens in sorted(H.PWG_BLOCK_SAMPLE_LENS.items()):
        inp = H.pwg_block_sample_inputs(blk.seed, m, R, A)
        aux = f64(inp["feats"]) @ blk.w["aux"].t()
        for d in H.PWG_BLOCK_DILATIONS:
            for first in (0, 1):
                with launched(kernel) if probe and kernel else contextlib.nullcontext():
                    x_out, sk = blk.run(inp["x"], inp["skips"], lens, d, first, fused, feats=inp["feats"])
                probe = False
                offs = np.concatenate([[0], np.cumsum(lens)])
                x_ref, s_ref, zmax, omax = blk.reference(inp["x"], inp["skips"], lens, d, first, [aux[offs[i] : offs[i + 1]] for i in range(len(lens))])
                tol_x, tol_s = blk.bounds(x_ref, zmax, omax)
                ex, es = max_abs(x_out, x_ref.numpy()), max_abs(sk, s_ref.numpy())
                assert ex <= tol_x and es <= tol_s, (m, d, first, ex, tol_x, es, tol_s)
                assert fused or max_abs(blk.x_f32, x_ref.numpy()) <= tol_x  # the four-launch path also carries x as fp32
                worst = [max(worst[0], ex / tol_x), max(worst[1], es / tol_s)]
    print("%s R=%d aux=%d k=%d: worst err / bound  x_out %.3f  skips %.3f" % (kernel or "four-launch", R, A, blk.plan.k, worst[0], worst[1]))


@pytest.mark.parametrize("r", [32, 96])
@pytest.mark.parametrize("aux", [20, 100])
@pytest.mark.parametrize("ksize", [3, 5])
def test_block_four_launch_path(voc, r, aux, ksize):
    """pre-split GEMM of ksize + 1 terms, pwg_gate_kernel, the projection GEMM, pwg_resid_kernel; row-major planes"""
    sweep_features_given(make_block(voc, r, aux, ksize, seed=H.PWG_BLOCK_SEEDS["four_launch"]), False, None)


@pytest.mark.parametrize("aux", [4, 32, 64])
def test_block_one_launch_small_aux(voc, aux):
    """pwg_layer_kernel<4,3>: 64 residual channels, aux <= 64, features given"""
    sweep_features_given(make_block(voc, 64, aux, seed=H.PWG_BLOCK_SEEDS["small_aux"]), True, "pwg_layer_kernel<4,3>")


@pytest.mark.parametrize("aux", [68, 80, 96])
def test_block_persistent_features_given(voc, aux):
    """pwg_layer_pkernel without the frame-rate term: ragged M (tail tile), utterance edges inside a tile (per-row segment bounds)"""
    sweep_features_given(make_block(voc, 64, aux, seed=H.PWG_BLOCK_SEEDS["persistent"]), True, "pwg_layer_pkernel")


def frame_rate_aux_terms(blk, mels):
    return [H.pwg_features_f64(blk.sd, m, blk.cfg) @ blk.w["aux"].t() for m in mels]


def frame_inputs(blk, lens, seed):
    return H.pwg_block_frame_inputs(seed, lens, blk.plan.hop, blk.plan.R, blk.plan.A)


@pytest.mark.parametrize("aux", [20, 80, 96])
@pytest.mark.parametrize("scales", [(2, 4, 4, 4), (4, 4, 4, 4), (4, 4, 4, 6)])
def test_block_persistent_frame_rate_term(voc, aux, scales):
    """pwg_layer_pkernel with the auxiliary term at frame rate (hop 128 / 256 / 384; aux 20 and 80 leave a partial last K-chunk in the projection):
    the operands come from _aux_frame_rate on random mels, the reference is conv_in on the replicate-padded utterance, the four stretch + smoothing
    stages and conv1x1_aux in float64, per utterance"""
    blk = make_block(voc, 64, aux, 3, scales, seed=H.PWG_BLOCK_SEEDS["frame_rate"])
    assert voc.aux_frame_rate(blk.plan)
    worst, probe = [0.0, 0.0], True
    for i, lens in enumerate(H.PWG_BLOCK_FRAME_LENS):
        mels, x, sk0 = frame_inputs(blk, lens, blk.seed + i)
        aux_terms = frame_rate_aux_terms(blk, mels)
        rows = [n * blk.plan.hop for n in lens]
        for d in H.PWG_BLOCK_DILATIONS:
            for first in (0, 1):
                with launched("pwg_layer_pkernel") if probe else contextlib.nullcontext():
                    x_out, sk = blk.run(x, sk0, lens, d, first, True, mels=mels)
                probe = False
                x_ref, s_ref, zmax, omax = blk.reference(x, sk0, rows, d, first, aux_terms)
                tol_x, tol_s = blk.bounds(x_ref, zmax, omax)
                ex, es = max_abs(x_out, x_ref.numpy()), max_abs(sk, s_ref.numpy())
                assert ex <= tol_x and es <= tol_s, (lens, d, first, ex, tol_x, es, tol_s)
                worst = [max(worst[0], ex / tol_x), max(worst[1], es / tol_s)]
    print("pwg_layer_pkernel/AUXF aux=%d hop=%d: worst err / bound  x_out %.3f  skips %.3f" % (aux, blk.plan.hop, worst[0], worst[1]))


@pytest.mark.parametrize("frame_rate", [True, False])
def test_block_capacity_form(voc, frame_rate):
    """pwg_layer_cap_pkernel, live < capacity, on the frame lists of the exact-size test with a dead tail of 5 frames.  The dead samples' x planes
    and skips are NaN patterns (and, with given features, the dead feature planes): never read -- a finite, correct result on every live sample
    -- and never written.  With the frame-rate term the dead FRAMES carry finite random mels: a live tile's 32-frame window may reach into them
    with zero coefficients, and 0 x NaN is NaN (include/fcl_hip.h, fcl_pwg_gather_pad)."""
    blk = make_block(voc, 64, 80, 3, (4, 4, 4, 4), seed=H.PWG_BLOCK_SEEDS["capacity"])
    probe, worst = True, [0.0, 0.0]
    for i, lens in enumerate(H.PWG_BLOCK_FRAME_LENS):
        cap = (sum(lens) + 5) * 256
        mels, x, sk0 = frame_inputs(blk, lens, blk.seed + i)
        rows = [n * 256 for n in lens]
        if frame_rate:
            aux_terms = frame_rate_aux_terms(blk, mels)
        else:
            feats = (2.5 * np.random.RandomState(blk.seed + 10 + i).standard_normal((sum(rows), 80))).astype(np.float32)
            aux = f64(feats) @ blk.w["aux"].t()
            offs = np.concatenate([[0], np.cumsum(rows)])
            aux_terms = [aux[offs[j] : offs[j + 1]] for j in range(len(rows))]
        for d in H.PWG_BLOCK_DILATIONS:
            for first in (0, 1):
                with launched("pwg_layer_cap_pkernel") if probe else contextlib.nullcontext():
                    if frame_rate:
                        x_out, sk = blk.run(x, sk0, lens, d, first, True, mels=mels, cap=cap)
                    else:
                        x_out, sk = blk.run(x, sk0, rows, d, first, True, feats=feats, cap=cap)
                probe = False
                x_ref, s_ref, zmax, omax = blk.reference(x, sk0, rows, d, first, aux_terms)
                tol_x, tol_s = blk.bounds(x_ref, zmax, omax)
                ex, es = max_abs(x_out, x_ref.numpy()), max_abs(sk, s_ref.numpy())
                assert ex <= tol_x and es <= tol_s, (lens, d, first, ex, tol_x, es, tol_s)
                worst = [max(worst[0], ex / tol_x), max(worst[1], es / tol_s)]
    print("pwg_layer_cap_pkernel frame_rate=%s: worst err / bound  x_out %.3f  skips %.3f" % (frame_rate, worst[0], worst[1]))


# ------------------------------------------------------------------------------------------------------------------ 5 whole generator
_GEN_CACHE = {}


def generator_reference(key, cfg, lens, seed):
    """float64 generator (exact) and the same on plane-rounded GEMM operands (the error model), per utterance, concatenated"""
    if key not in _GEN_CACHE:
        sd, mels, noise = H.pwg_generator_inputs(seed, lens, cfg)
        ref = [H.pwg_generator_f64(sd, m, z, cfg) for m, z in zip(mels, noise)]
        mod = [H.pwg_generator_f64(sd, m, z, cfg, rnd=H.plane_round) for m, z in zip(mels, noise)]
        nl = len(ref[0]["taps"])
        cat = lambda rs: dict(taps=[torch.cat([r["taps"][l] for r in rs]) for l in range(nl)], skips=torch.cat([r["skips"] for r in rs]),
                              wav=[r["wav"] for r in rs])
        _GEN_CACHE[key] = (sd, mels, noise, cat(ref), cat(mod))
    return _GEN_CACHE[key]


def check_generator(voc, key, cfg, lens, seed, kernels):
    sd, mels, noise, ref, mod = generator_reference(key, cfg, lens, seed)
    gen = voc.ParallelWaveGANGenerator(voc.PWGPlan(sd, DEV, cfg))
    with launched(*kernels):
        got, aux = gen.synthesize(mels, noise=noise, return_intermediates=True)
    torch.cuda.synchronize()
    rows = []
    bad = []
    for l, (t_ref, t_mod) in enumerate(zip(ref["taps"], mod["taps"])):
        e_gpu, e_mod = max_abs(aux["taps"][l].cpu().double(), t_ref), max_abs(t_mod, t_ref)
        bound = 4 * max(e_mod, 2.0 ** -15 * float(t_ref.abs().max()))
        rows.append((l, e_gpu, e_mod, bound))
        if not e_gpu <= bound:
            bad.append((l, e_gpu, bound))
    e_gpu, e_mod = max_abs(aux["skips"].cpu().double(), ref["skips"]), max_abs(mod["skips"], ref["skips"])
    s_bound = 4 * max(e_mod, 2.0 ** -15 * float(ref["skips"].abs().max()))
    print("%s: tap  err_gpu  err_model  bound" % key)
    for r in rows:
        print("  %2d  %.3e  %.3e  %.3e" % r)
    print("  skip sum  %.3e  %.3e  %.3e" % (e_gpu, e_mod, s_bound))
    wav_rows = []
    for g, w_ref, w_mod in zip(got, ref["wav"], mod["wav"]):
        peak = float(w_ref.abs().max())
        e, em = max_abs(g.cpu().double(), w_ref), max_abs(w_mod, w_ref)
        wav_rows.append((e, em, peak))
        print("  waveform  %.3e  %.3e  peak %.3f" % (e, em, peak))
    assert not bad, bad
    assert e_gpu <= s_bound
    for e, em, peak in wav_rows:
        assert e <= 1e-3 * peak and e <= 4 * max(em, 2.0 ** -15 * peak)


@pytest.mark.parametrize("switch", ["default", "FCL_PWG_FUSED=0", "FCL_PWG_AUX_FRAME_RATE=0"])
def test_generator_v1_every_tap_vs_float64(voc, monkeypatch, switch):
    """v1 geometry on random weights at a gain that saturates the gates: every block's tap, the skip sum and the waveform against float64;
    bound = 4 x max(error of the float64 generator on plane-rounded operands, plane storage) -- the measured figures are in DESIGN.md 6b"""
    if switch != "default":
        monkeypatch.setenv(*switch.split("="))
    kernels = {"default": ["pwg_layer_pkernel", "pwg_last_kernel"], "FCL_PWG_FUSED=0": ["pwg_last_kernel"], "FCL_PWG_AUX_FRAME_RATE=0": ["pwg_layer_pkernel"]}[switch]
    check_generator(voc, "v1", None, H.PWG_GENERATOR_LENS, H.PWG_GENERATOR_SEEDS["v1"], kernels)


def test_generator_small_aux_every_tap_vs_float64(voc):
    """64 residual channels, aux 32, hop 6: thirty pwg_layer_kernel<4,3> blocks with ragged tiles and a one-frame utterance"""
    check_generator(voc, "small", H.PWG_SMALL_CFG, H.PWG_SMALL_LENS, H.PWG_GENERATOR_SEEDS["small"], ["pwg_layer_kernel<4,3>", "pwg_last_kernel"])


@pytest.mark.parametrize("switch", ["default", "FCL_PWG_AUX_FRAME_RATE=0"])
def test_generator_v1_many_tiles_per_workgroup_vs_float64(voc, monkeypatch, switch):
    """291 frames = 582 tiles of 128 samples: pwg_layer_pkernel runs one workgroup per compute unit, so each walks two or three tiles -- the next
    tile's bounds and first chunks are requested during the epilogue and the ring slot carries over (7 chunks per tile on a 3-deep ring with the
    frame-rate term, 9 without).  Same bound as the 70-frame case."""
    if switch != "default":
        monkeypatch.setenv(*switch.split("="))
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert sum(H.PWG_LONG_LENS) * 2 > n_cu, "the case needs more tiles than compute units"
    check_generator(voc, "long", None, H.PWG_LONG_LENS, H.PWG_GENERATOR_SEEDS["long"], ["pwg_layer_pkernel", "pwg_last_kernel"])


# ------------------------------------------------------------------------------------------------------------------ 6 FCL_GEMM_BF16
BF16_GEMM = 2e-5  # test_bf16_gemm_mode_rounds_both_operands_and_accumulates_in_fp32: fp32 accumulation of exactly representable products


def check_bf16_block(blk, run_kwargs, rows, aux_terms_exact, aux_terms_rounded, kernel, x, sk0, lens):
    from fcl_taco2_amd import _lib, ops

    d, first = 2, 0
    with ops.gemm_mode("bf16"):
        assert lib().fcl_get_gemm_mode() == _lib.GEMM_BF16
        with launched(kernel + "/bf16"):
            x_out, sk = blk.run(x, sk0, lens, d, first, True, **run_kwargs)
    assert lib().fcl_get_gemm_mode() == _lib.GEMM_F32
    if callable(aux_terms_rounded):  # read from the operand buffers of the run just made
        aux_terms_rounded = aux_terms_rounded()
    x_ref, s_ref, zmax, omax = blk.reference(x, sk0, rows, d, first, aux_terms_rounded, rnd=H.bf16_round)
    tol_x, tol_s = blk.bounds(x_ref, zmax, omax, gemm=BF16_GEMM)
    ex, es = max_abs(x_out, x_ref.numpy()), max_abs(sk, s_ref.numpy())
    x_exact, s_exact, _, omax_e = blk.reference(x, sk0, rows, d, first, aux_terms_exact)
    dx, ds = max_abs(x_out, x_exact.numpy()), max_abs(sk, s_exact.numpy())
    print("%s/bf16: x_out %.3g / %.3g  skips %.3g / %.3g; from the exact block %.3g, %.3g (scale %.3g)" % (kernel, ex, tol_x, es, tol_s, dx, ds, omax_e))
    assert ex <= tol_x and es <= tol_s
    assert min(dx, ds) > 1e-4 * max(1.0, omax_e)  # really the rounded operands


@pytest.mark.parametrize("aux,kernel", [(32, "pwg_layer_kernel<4,3>"), (80, "pwg_layer_pkernel")])
def test_bf16_mode_block_features_given(voc, aux, kernel):
    """reference: the float64 block on bf16-ROUNDED x, features, weights and gate output"""
    blk = make_block(voc, 64, aux, seed=H.PWG_BLOCK_SEEDS["bf16"])
    lens = H.PWG_BLOCK_SAMPLE_LENS[700]
    inp = H.pwg_block_sample_inputs(blk.seed, 700, 64, aux)
    offs = np.concatenate([[0], np.cumsum(lens)])
    split = lambda a: [a[offs[i] : offs[i + 1]] for i in range(len(lens))]
    exact = f64(inp["feats"]) @ blk.w["aux"].t()
    rounded = H.bf16_round(f64(inp["feats"])) @ H.bf16_round(blk.w["aux"]).t()
    check_bf16_block(blk, dict(feats=inp["feats"]), lens, split(exact), split(rounded), kernel, inp["x"], inp["skips"], lens)


def frame_rate_term_from_operands(blk, M, hi_only):
    """The auxiliary term as the kernel contracts it, in float64 from the operand buffers of the last Block.run: coefficient line of sample m x the
    32-frame window of the projected features (pt_a when 2 <= f mod 32 <= 29, else pt_b; include/fcl_hip.h).  hi_only: the bf16-rounded operands
    (the hi words); else hi + lo."""
    kp, pt_a, pt_b, ld_pt = blk.fr
    hop, G = blk.plan.hop, 2 * blk.plan.R
    val = (lambda raw: bf16_to_f32(raw[..., 0, :]).astype(np.float64)) if hi_only else planes_value
    k = val(kp.cpu().numpy().view(np.uint16).reshape(-1, 2, 32))[:M]
    pa = val(planes_np(pt_a[:G], G)).reshape(G, ld_pt * 32)
    pb = val(planes_np(pt_b[:G], G)).reshape(G, ld_pt * 32)
    out = np.zeros((M, G))
    for f in range(M // hop):
        r = f & 31
        win = pa[:, (f >> 5) * 32 :][:, :32] if 2 <= r <= 29 else pb[:, ((f + 16) >> 5) * 32 :][:, :32]
        out[f * hop : (f + 1) * hop] = k[f * hop : (f + 1) * hop] @ win.T
    return torch.from_numpy(out)


@pytest.mark.parametrize("cap", [False, True])
def test_bf16_mode_block_frame_rate_term(voc, cap):
    """pwg_layer_pkernel / pwg_layer_cap_pkernel with the frame-rate term in bf16 mode.  The rounded operands of the auxiliary chunk are the
    coefficient lines and the projected features: the reference contracts the hi words of exactly those operand buffers (their producers are pinned
    by test_aux_coeff_lines_bit_for_bit and test_gpu_planes.py) in float64; x, the taps, the gate output and W_os are bf16-rounded as above."""
    blk = make_block(voc, 64, 80, 3, (4, 4, 4, 4), seed=H.PWG_BLOCK_SEEDS["bf16_frame_rate"])
    lens = [3, 1, 33, 2]
    mels, x, sk0 = frame_inputs(blk, lens, blk.seed + 1)
    rows = [n * 256 for n in lens]
    M = sum(rows)
    kw = dict(mels=mels, cap=M + 4 * 256) if cap else dict(mels=mels)
    blk.run(x, sk0, lens, 2, 0, True, **kw)  # fills blk.fr in the fp32-equivalent mode
    offs = np.concatenate([[0], np.cumsum(rows)])
    split = lambda a: [a[offs[i] : offs[i + 1]] for i in range(len(rows))]
    full = frame_rate_term_from_operands(blk, M, False)
    exact = frame_rate_aux_terms(blk, mels)
    assert max_abs(full, torch.cat(exact)) <= 3e-5 * max(1.0, float(torch.cat(exact).abs().max()))  # the operand reading itself, against float64
    check_bf16_block(blk, kw, rows, exact, lambda: split(frame_rate_term_from_operands(blk, M, True)),
                     "pwg_layer_cap_pkernel" if cap else "pwg_layer_pkernel", x, sk0, lens)


@pytest.mark.parametrize("cap", [False, True])
def test_bf16_mode_last_stage(voc, cap):
    """pwg_last_kernel / pwg_last_cap_kernel on bf16-rounded ReLU(skips * scale) and W1"""
    from fcl_taco2_amd import ops

    m = 1000 if not cap else 1024
    mc = m + 512 if cap else m
    sk, w1, b1, w2, b2, scale = last_stage_inputs(64, m, 800 + cap)
    skd = torch.full((mc, 64), float("nan"), device=DEV)
    skd[:m] = dev(sk)
    w1p, b1d, w2d = ops.pack_planes(dev(w1)), dev(b1), dev(w2)
    wav = Guarded(mc, torch.float32)
    name = "pwg_last_cap_kernel/bf16" if cap else "pwg_last_kernel/bf16"
    with ops.gemm_mode("bf16"), launched(name):
        if cap:
            live = dev(np.array([m // 256, m, 0, 1], dtype=np.int32))
            chk(lib().fcl_pwg_last_cap_fwd(skd.data_ptr(), scale, w1p.data_ptr(), b1d.data_ptr(), w2d.data_ptr(), b2, wav.t.data_ptr(), mc, 64, live.data_ptr(), stream()))
        else:
            chk(lib().fcl_pwg_last_fwd(skd.data_ptr(), scale, w1p.data_ptr(), b1d.data_ptr(), w2d.data_ptr(), b2, None, None, wav.t.data_ptr(), m, 64, stream()))
    # the device rounds fp32(skips * scale): round the reference's product the same way (one fp32 rounding first)
    y32 = torch.relu((torch.from_numpy(sk) * np.float32(scale)))
    h = H.bf16_round(y32.double()) @ H.bf16_round(f64(w1)).t() + f64(b1)
    ref = torch.relu(h) @ f64(w2) + b2
    _, h_exact, exact = last_stage_ref(sk, w1, b1, w2, b2, scale)
    got = wav.t[:m].cpu().numpy()
    err, tol, diff = max_abs(got, ref.numpy()), last_stage_tol(h, w2, BF16_GEMM), max_abs(got, exact.numpy())
    print("%s: err %.3g tol %.3g, from the exact stage %.3g" % (name, err, tol, diff))
    assert err <= tol and diff > 1e-4 * max(1.0, float(exact.abs().max()))
    assert wav.intact() and wav.untouched(wav.t[m:])


def test_capacity_last_stage_vs_float64(voc):
    """pwg_last_cap_kernel in the default mode: live < capacity, dead skips are NaN and the dead waveform samples stay untouched"""
    from fcl_taco2_amd import ops

    m, mc = 768, 1280
    sk, w1, b1, w2, b2, scale = last_stage_inputs(64, m, 900)
    skd = torch.full((mc, 64), float("nan"), device=DEV)
    skd[:m] = dev(sk)
    w1p, b1d, w2d = ops.pack_planes(dev(w1)), dev(b1), dev(w2)
    wav = Guarded(mc, torch.float32)
    live = dev(np.array([m // 256, m, 0, 1], dtype=np.int32))
    with launched("pwg_last_cap_kernel"):
        chk(lib().fcl_pwg_last_cap_fwd(skd.data_ptr(), scale, w1p.data_ptr(), b1d.data_ptr(), w2d.data_ptr(), b2, wav.t.data_ptr(), mc, 64, live.data_ptr(), stream()))
    _, h, ref = last_stage_ref(sk, w1, b1, w2, b2, scale)
    assert max_abs(wav.t[:m].cpu().numpy(), ref.numpy()) <= last_stage_tol(h, w2)
    assert wav.intact() and wav.untouched(wav.t[m:])
