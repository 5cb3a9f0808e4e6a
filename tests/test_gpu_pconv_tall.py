"""-m gpu: the 256-row and the 96-column tiles of the Conv1d stencil (gemm_planes.hip pconv_kernel<4,2,4,4>, <4,2,4,3>, <4,2,2,3>) through ops.conv1d_planes.

The library reads its tunables once per process, so the launches run in child processes of this file (`python test_gpu_pconv_tall.py MODE OUT`), one per
selection, each running every case once and saving its buffers; the tests below read what the children saved:
    tall  FCL_PCONV_TALL_MIN=1                                            Cout 128 / 160 -> <4,2,4,4>, Cout 80 -> <4,2,4,3>
    old   FCL_PCONV_TALL_MIN=0   FCL_PCONV_N96_MIN=0 FCL_PCONV_BIG_MIN=1      the tiles they replace: Cout 128 / 160 -> <4,2,2,4>, Cout 80 -> <2,2,2,2> (two 64-column tiles)
    mid   FCL_PCONV_TALL_MIN=100 FCL_PCONV_N96_MIN=1 FCL_PCONV_BIG_MIN=1      Cout 80 with too few 256-row tiles -> <4,2,2,3> (the Cout 80 cases only)

M = 530 = two full 256-row tiles + 18 rows, k = 5; utterance boundaries at rows 254 .. 258 (inside the halo on both sides of the tile edge at 256), which
makes four 1-row utterances, and one 3-row utterance, all shorter than the padding; Cin 80 (zero-padded last 128-byte line) / 128; Cout 128, 160 (second
column tile partial), 80 (96-column form, planes' padding columns); device row count absent / 530 / 300 (300: tile 1 computed whole, tile 2 skipped).

Per case: (1) the launched kernel, from the library's launch record; (2) fp32 output within 3e-5 of a float64 NumPy convolution of the fp32 inputs (the bound
of tests/test_gpu_planes.py for this op, unscaled as there: outputs are O(1)), planes within 2^-15 * max(1, |y|max) of the fp32 output (that file's bound for
planes against their fp32 twin) with zero padding columns; (3) bit equality, fp32 and planes, with the child that ran the old tiles, on the rows both wrote;
(4) every buffer is allocated between guard lines and pre-filled with a NaN bit pattern: the guards and the rows of skipped tiles keep it."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, KSZ = 530, 5
SEG_LENS = [254, 1, 1, 1, 1, 3, 120, 149]  # ends at 254, 255, 256, 257, 258, 261, 381, 530
CINS, COUTS, MDEVS = (80, 128), (128, 160, 80), (None, 530, 300)
FORMS = ("tanh_planes", "none_res_f32")  # tanh, planes (+ fp32) out | no activation, residual, fp32 out
GUARD_BYTES = 1024
NAN32, NAN16 = 0x7FC00000, 0x7FC0  # quiet NaN as fp32 / as a bf16 half-word
ENVS = {"tall": dict(FCL_PCONV_TALL_MIN="1"), "old": dict(FCL_PCONV_TALL_MIN="0", FCL_PCONV_N96_MIN="0", FCL_PCONV_BIG_MIN="1"),
        "mid": dict(FCL_PCONV_TALL_MIN="100", FCL_PCONV_N96_MIN="1", FCL_PCONV_BIG_MIN="1")}
CASES = [(ci, co, md, f) for ci in CINS for co in COUTS for md in MDEVS for f in FORMS]


def case_id(case):
    ci, co, md, f = case
    return "cin%d_cout%d_mdev%s_%s" % (ci, co, "none" if md is None else md, f)


def segments():
    assert sum(SEG_LENS) == M
    starts = np.cumsum([0] + SEG_LENS[:-1])
    lo = np.repeat(starts, SEG_LENS).astype(np.int32)
    return lo, (lo + np.repeat(SEG_LENS, SEG_LENS)).astype(np.int32)


def inputs(cin, cout):
    """x [M, cin], w [cout, cin, k] (unit-variance pre-activations), bias, residual: the same arrays in the children and in the reference."""
    rng = np.random.RandomState(1000 * cin + cout)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    return f(M, cin), f(cout, cin, KSZ) / np.float32(np.sqrt(cin * KSZ)), f(cout), f(M, cout)


def expected_kernel(mode, cout):
    if cout == 80:
        return {"tall": "pconv_kernel<4,2,4,3,2>", "old": "pconv_kernel<2,2,2,2,2>", "mid": "pconv_kernel<4,2,2,3,2>"}[mode]
    return {"tall": "pconv_kernel<4,2,4,4,2>", "old": "pconv_kernel<4,2,2,4,2>", "mid": "pconv_kernel<4,2,2,4,2>"}[mode]


def tile_rows(kernel):
    wm, _, tm = [int(v) for v in kernel[kernel.index("<") + 1:].split(",")[:3]]
    return 16 * wm * tm


def rows_written(kernel, m_dev):
    """Tiles that start below the device's row count are computed whole (up to M), the others are skipped."""
    bm = tile_rows(kernel)
    return M if m_dev is None else min(M, (m_dev + bm - 1) // bm * bm)


# ------------------------------------------------------------------------------------------------------------------------------ child process
def child_main(mode, out_path):
    import torch

    sys.path.insert(0, ROOT)
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib, ops

    _lib.load()
    assert ops.planes_enabled()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")  # noqa: E731
    real_empty = torch.empty
    made = []

    def guarded_empty(*shape, **kw):
        """torch.empty for the op's outputs: a view into a buffer with a guard line on either side, everything pre-filled with the NaN pattern."""
        shape = tuple(shape[0]) if len(shape) == 1 and not isinstance(shape[0], int) else shape
        dtype = kw["dtype"]
        item, pat, idt = (4, NAN32, torch.int32) if dtype == torch.float32 else (2, NAN16, torch.int16)
        assert dtype in (torch.float32, torch.int16)
        g, n = GUARD_BYTES // item, int(np.prod(shape))
        buf = torch.full((n + 2 * g,), pat, device=kw["device"], dtype=idt)
        made.append(buf)
        return buf[g: g + n].view(dtype).view(*shape)

    lo_np, hi_np = segments()
    lo, hi = dev(lo_np), dev(hi_np)
    saved = {}
    for cin in CINS:
        for cout in COUTS:
            if mode == "mid" and cout != 80:
                continue
            x, w, b, res = inputs(cin, cout)

            class CV(object):
                pass

            cv = CV()
            taps = dev(w).permute(2, 0, 1).contiguous().reshape(KSZ * cout, cin)  # tap-major [k * Cout, Cin]
            cv.wpp, cv.bias, cv.cin, cv.cout, cv.k = ops.pack_planes(taps), dev(b), cin, cout, KSZ
            xp, res_d = ops.pack_planes(dev(x)), dev(res)
            for md in MDEVS:
                m_dev = None if md is None else dev(np.array([md], np.int32))
                for form in FORMS:
                    del made[:]
                    _lib.prof_enable(True)
                    torch.empty = guarded_empty
                    try:
                        if form == "tanh_planes":
                            ops.conv1d_planes(xp, cv, lo, hi, ops.ACT_TANH, want_f32=True, want_planes=True, m_dev=m_dev)
                        else:
                            ops.conv1d_planes(xp, cv, lo, hi, ops.ACT_NONE, residual=res_d, want_f32=True, want_planes=False, m_dev=m_dev)
                    finally:
                        torch.empty = real_empty
                    torch.cuda.synchronize()
                    names = sorted(_lib.prof_collect())
                    _lib.prof_enable(False)
                    key = case_id((cin, cout, md, form))
                    saved[key + "__kernels"] = np.array(names)
                    saved[key + "__y"] = made[0].cpu().numpy()  # int32 words, guards included
                    if form == "tanh_planes":
                        saved[key + "__yp"] = made[1].cpu().numpy()  # int16 half-words, guards included
    np.savez(out_path, **saved)


# ---------------------------------------------------------------------------------------------------------------------------------- the tests
@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    import torch

    assert torch.cuda.is_available()
    if os.environ.get("FCL_PRECISION", "1") == "0" or os.environ.get("FCL_PLANES", "1") == "0":
        pytest.skip("FCL_PRECISION=0 / FCL_PLANES=0: the pre-split operand path is off")
    out = {}
    d = tmp_path_factory.mktemp("pconv_tall")
    for mode, extra in ENVS.items():
        path = str(d / (mode + ".npz"))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), mode, path], env=dict(os.environ, **extra), cwd=ROOT, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, "the %s child failed:\n%s" % (mode, "\n".join((r.stdout + "\n" + r.stderr).strip().splitlines()[-25:]))
        out[mode] = dict(np.load(path))
    return out


_REF = {}


def reference(cin, cout, form):
    """float64 convolution of the fp32 inputs with zero padding at the utterance ends; computed once per (Cin, Cout, form)."""
    if (cin, cout, form) not in _REF:
        x, w, b, res = inputs(cin, cout)
        lo, hi = segments()
        t = np.arange(M)
        acc = np.zeros((M, cout))
        for j in range(KSZ):
            src = t + j - (KSZ - 1) // 2
            ok = (src >= lo) & (src < hi)
            xs = np.where(ok[:, None], x[np.clip(src, 0, M - 1)].astype(np.float64), 0.0)
            acc += xs @ w[:, :, j].astype(np.float64).T
        acc += b
        _REF[(cin, cout, form)] = np.tanh(acc) if form == "tanh_planes" else acc + res
    return _REF[(cin, cout, form)]


def split_guards(words, n, pattern):
    g = len(words) - n
    assert g % 2 == 0 and g > 0
    g //= 2
    assert (words[:g] == pattern).all() and (words[g + n:] == pattern).all(), "a guard line was overwritten"
    return words[g: g + n]


def bf16_words_to_f64(u16):
    return (u16.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def check_child(run, mode, case):
    cin, cout, md, form = case
    key = case_id(case)
    kernels = list(run[key + "__kernels"])
    assert kernels == [expected_kernel(mode, cout)], kernels
    live = rows_written(kernels[0], md)
    ref = reference(cin, cout, form)
    nan32 = np.int32(NAN32)
    yw = split_guards(run[key + "__y"], M * cout, nan32).reshape(M, cout)
    assert (yw[live:] == nan32).all(), "rows of a skipped tile were written"
    y = yw[:live].view(np.float32)
    assert np.isfinite(y).all()
    err = float(np.max(np.abs(y.astype(np.float64) - ref[:live])))
    print("%s %s %s: rows %d, max |y - ref| = %.3g" % (mode, key, kernels[0], live, err))
    assert err < 3e-5
    out = [yw[:live]]
    if form == "tanh_planes":
        lines = (cout + 31) // 32
        nan16 = np.int16(NAN16)
        pw = split_guards(run[key + "__yp"], M * lines * 64, nan16).reshape(M, lines, 2, 32)
        assert (pw[live:] == nan16).all(), "plane rows of a skipped tile were written"
        pu = pw[:live].view(np.uint16)
        val = (bf16_words_to_f64(pu[:, :, 0, :]) + bf16_words_to_f64(pu[:, :, 1, :])).reshape(live, lines * 32)
        assert np.max(np.abs(val[:, :cout] - y.astype(np.float64))) < 2.0 ** -15 * max(1.0, float(np.abs(y).max()))
        assert not pu.transpose(0, 1, 3, 2).reshape(live, lines * 32, 2)[:, cout:].any()  # zero padding past Cout in both planes
        out.append(pw[:live])
    return out


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_tall_and_96_column_tiles(runs, case):
    """The 256-row tile (Cout 128 / 160) or the 256 x 96 tile (Cout 80): kernel, fp64 reference, guards and sentinels, and bit equality with the old tiles."""
    new, old = check_child(runs["tall"], "tall", case), check_child(runs["old"], "old", case)
    for a, b in zip(new, old):
        both = min(len(a), len(b))  # (with a device row count of 300 the old tiles stop at row 320 / 384, the tall ones at 512)
        assert both >= (case[2] or M) and np.array_equal(a[:both], b[:both])


@pytest.mark.parametrize("case", [c for c in CASES if c[1] == 80], ids=[case_id(c) for c in CASES if c[1] == 80])
def test_128_row_96_column_tile(runs, case):
    """Cout 80 with too few 256-row tiles: pconv_kernel<4,2,2,3>, the same four checks."""
    new, old = check_child(runs["mid"], "mid", case), check_child(runs["old"], "old", case)
    for a, b in zip(new, old):
        both = min(len(a), len(b))
        assert both >= (case[2] or M) and np.array_equal(a[:both], b[:both])


if __name__ == "__main__":
    child_main(sys.argv[1], sys.argv[2])
