"""-m gpu: every kernel form behind fcl_lstm_step_fwd against the float64 statement of the step (tests/lstm_step_ref.py), one call per case.

Every case compares h, c and each requested side output (save_gates, save_c_new, save_c_old, save_h_old, out2) with the reference within its
PER-ELEMENT bound (lstm_step_ref.lstm_step_bound: the 3e-5 GEMM bound carried through the float64 cell; an element that is a copy -- a dead row,
a kept zoneout element, the saved old state -- must match exactly), and asserts
  * the launched kernel, from the library's launch record: a later threshold change cannot silently stop a form from being tested;
  * guard lines of an all-ones (NaN) bit pattern in front of and behind every written buffer;
  * rows from min(M, *m_dev) on keep what the buffers held, in every output;
  * h_out_p, where requested, equals helpers.split_planes_np(h_out) bit for bit.
It prints the worst error / bound ratio per output (HISTORY.md records them per kernel form).

Shapes: the smallest M at which launch_lstm_step / lstm_step_is_small (gemm_f32.hip), launch_lstm_small (decoder_step.hip) and launch_lstm_planes /
launch_plstm_lw (gemm_planes.hip) select each form under the default tunables, one row past a tile multiple (lstm_step_ref.FAMILIES); option sets:
lstm_step_ref.OPTIONS.  The inputs and the bound are checked without a GPU in tests/test_lstm_step_ref_cpu.py.  Under FCL_PRECISION=0 (read once
per process) a child pytest runs the smallest lstm_small_ff_kernel/f32 and two plstm_kernel<...>/f32 cases at the same bound."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lstm_step_ref as R
from helpers import split_planes_np

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = os.environ.get("FCL_PRECISION", "1") == "0"
GUARD = 256  # elements of guard in front of and behind every written buffer (>= 512 bytes: buffers stay 128-byte aligned)
torch.set_num_threads(min(16, torch.get_num_threads()))
try:  # numpy's BLAS threads of the float64 contractions, where the pool can be bounded from here
    from threadpoolctl import threadpool_limits
except ImportError:
    threadpool_limits = None

SMALL, SMALL_X3, SMALL_FF = "lstm_small_kernel", "lstm_small_kernel/bf16x3", "lstm_small_ff_kernel/f32"
STEP_14, STEP_22, STEP_41, STEP_TM2 = ("lstm_step_kernel<%s,{mode},1,%d>/bf16x3" % t for t in (("1,4", 1), ("2,2", 1), ("4,1", 1), ("2,2", 2)))
P_2214, P_2223, P_4222, P_2124, P_4223 = ("plstm_kernel<%s,{mode},4>" % t for t in ("2,2,1,4", "2,2,2,3", "4,2,2,2", "2,1,2,4", "4,2,2,3"))
ALL = ("l0", "l1", "l0z", "l1z", "gen", "genz", "bilstm", "train0", "train1", "kd")
FIXED = ("l0", "l1", "l0z", "l1z")

# id: (family, operand kind, kernel, kernel of the options with masks / saved gates (the wide / training thresholds) or None, options,
#      options also run with a device row count below M, leading-dimension padding in elements)
# kinds: f32 = A / W only; frag = + fragment-major bf16 planes of W; ff = + fragment-major fp32 W; planes = + P32 planes of A and W;
#        planes_only = the planes alone, A / W NULL
CASES = {
    "f32_m1": ("m1", "f32", SMALL, None, ("l0", "l1", "l0z", "gen", "train1"), (), 0),
    "f32_m17": ("m17", "f32", SMALL, None, ALL, FIXED, 0),
    "f32_u24_m17": ("u24_m17", "f32", SMALL, None, ("l1", "l1z", "gen", "bilstm", "train1"), (), 4),   # U % 16 != 0, K = 36, lda = ldw = 40
    "f32_t3_m17": ("t3_m17", "f32", SMALL, None, ("l0", "l1", "gen", "train0", "kd"), (), 4),          # three terms, lda / ldw > K
    "f32_m513": ("m513", "f32", STEP_14, None, ALL, ("l0", "l1"), 0),
    "f32_t3_m513": ("t3_m513", "f32", STEP_14, None, ("l0", "gen", "train1"), (), 4),
    "f32_m737": ("m737", "f32", STEP_22, None, ("l0", "l1", "gen", "bilstm", "train0"), ("l1",), 0),
    "f32_u24_m513": ("u24_m513", "f32", STEP_22, None, ("l1", "gen", "bilstm", "train1"), (), 4),
    "f32_u16_m513": ("u16_m513", "f32", STEP_41, None, ("l0", "l1", "gen", "bilstm", "train0", "kd"), ("l0",), 0),
    "f32_m961": ("m961", "f32", STEP_TM2, None, ("l0", "l1", "l0z", "gen", "bilstm", "train1", "kd"), ("l0", "l1"), 0),
    "f32_wide_m65": ("wide_m65", "f32", STEP_14, None, ("l0", "l1", "gen", "train1"), (), 0),            # U = 1024: the small-step bound is 64 rows
    "frag_m17": ("m17", "frag", SMALL_X3, None, ALL, FIXED, 0),                                           # register-resident: two K = 256 terms / one
    "frag_u32_m70": ("u32_m70", "frag", SMALL_X3, None, ("l0", "l1", "l0z", "l1z", "gen", "bilstm", "train0", "train1", "kd"), ("l0", "l1z"), 0),  # general K
    "ff_m17": ("m17", "ff", SMALL_FF, None, ("l0", "l1", "l0z", "l1z", "gen", "bilstm", "train1", "kd"), ("l0", "l1z"), 0),
    "ponly_m17": ("m17", "planes_only", P_2214, P_2214, ("l0", "l1", "l0z", "l1z", "gen", "bilstm"), ("l0",), 0),
    "p_m520": ("m520", "planes", P_2214, P_2214, ALL, FIXED, 0),
    "p_m600": ("m600", "planes", P_2223, P_2214, ("l0", "l1", "l0z", "l1z", "gen", "kd"), FIXED, 0),
    "p_m1930": ("m1930", "planes", P_4222, P_2223, ALL, FIXED, 0),
    "p_m1200": ("m1200", "planes", None, P_2124, ("train0", "train1"), (), 0),
    "p_m2310": ("m2310", "planes", None, P_4223, ("train0", "train1"), (), 0),
    "p_wide_m65": ("wide_m65", "planes", P_2214, P_2214, ("l0", "l1", "gen", "train1"), (), 0),
    "p_k260": ("k260_m520", "planes", P_2214, P_2214, ("l0", "l1", "gen", "train0"), (), 1),             # K = 260; lda_p one line more than needed
}
EXACT_CHILD = ("ff_m17", "p_m520", "p_m600")  # what the FCL_PRECISION=0 child runs (there the "planes" cases pass fp32 rows: the exact-line kernels)
PARAMS = [(cid, opt, live) for cid, c in CASES.items() for opt in c[4] for live in ((False, True) if opt in c[5] else (False,))]


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return t.to(DEV).contiguous()


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib

    _lib.load()
    return _lib


def guarded(shape, dtype, fill):
    """(whole allocation, view of `shape` filled with `fill`): GUARD elements of all-ones bits (a NaN for float32) on either side of the view"""
    n = int(np.prod(shape))
    full = torch.empty(2 * GUARD + n, device=DEV, dtype=dtype)
    full.view(torch.int32 if dtype == torch.float32 else torch.int16).fill_(-1)
    view = full[GUARD: GUARD + n].view(*shape)
    view.fill_(fill)
    assert view.data_ptr() % 128 == 0
    return full, view


def guards_intact(full):
    raw = full.view(torch.int32 if full.dtype == torch.float32 else torch.int16)
    return bool((raw[:GUARD] == -1).all()) and bool((raw[-GUARD:] == -1).all())


def padded(x, pad):
    """device copy of x [R, K] with row stride K + pad; the padding holds NaN (it must not be read)"""
    if not pad:
        return dev(x), x.shape[1]
    buf = torch.full((x.shape[0], x.shape[1] + pad), float("nan"), device=DEV)
    buf[:, : x.shape[1]] = dev(x)
    return buf, x.shape[1] + pad


class Operands(object):
    """The terms of a family on the device in the forms of `kind`, and everything else any option set reads."""

    def __init__(self, _lib, ops, inp, kind, pad):
        self.keep, self.terms = [], []
        if EXACT and kind in ("planes", "frag"):
            kind = "f32"  # (the exact-fp32 process has no bf16 forms)
        for a, w in inp["terms"]:
            k = a.shape[1]
            fpad = pad if kind == "f32" else 0
            (A, lda), (W, ldw) = padded(a, fpad), padded(w, fpad)
            whi = wlo = wff = ap = wp = None
            lda_p = ldw_p = (k + 31) // 32
            if kind == "frag":
                whi, wlo = ops.pack_frag_bf16(W)
            if kind == "ff":
                wff = ops.pack_frag_f32(W)
            if kind in ("planes", "planes_only"):
                ap, wp = ops.pack_planes(A), ops.pack_planes(W)
                if pad:  # rows of lda_p + pad lines; the extra lines hold NaN halves
                    wide = torch.full((a.shape[0], (lda_p + pad) * 64), 0x7FC0, device=DEV, dtype=torch.int16)
                    wide[:, : lda_p * 64] = ap
                    ap, lda_p = wide, lda_p + pad
                    assert ap.data_ptr() % 128 == 0
            self.keep += [A, W, whi, wlo, wff, ap, wp]
            p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
            f32 = kind != "planes_only"
            self.terms.append(_lib.GemmTerm(p(A) if f32 else None, p(W) if f32 else None, lda, ldw, k, 0, p(whi), p(wlo), p(ap), p(wp), lda_p, ldw_p, 0, p(wff)))
        self.side = {k: dev(inp[k]) for k in ("h_in", "c_in", "g", "g_t", "bias", "wpos", "dur", "row_len", "keep_h", "keep_c", "frame_off")}


_state = {}


def family_state(_lib, ops, cid):
    """inputs, device operands and the float64 contractions of one case id (one at a time: parametrisation runs a case's options together)"""
    if _state.get("cid") != cid:
        _state.clear()
        fam, kind, _, _, _, _, pad = CASES[cid]
        inp = R.family_inputs(fam)
        _state.update(cid=cid, inp=inp, ops=Operands(_lib, ops, inp, kind, pad), mm={})
    return _state


def expected_kernel(cid, opt, zero):
    _, kind, kern, kern_train, _, _, _ = CASES[cid]
    o = R.OPTIONS[opt]
    training = bool(o.get("masks") or o.get("save"))
    name = kern_train if training and kern_train else kern
    layer = 0 if (o.get("g") and o.get("pos") and not o.get("bias")) else 1 if (o.get("bias") and not o.get("g") and not o.get("pos")) else -1
    if name.startswith("plstm"):  # launch_plstm_lw: the fixed modes take no mask, row_len, saved gates or out2; + 2 in the zero-state form
        plain = not (o.get("masks") or o.get("row_len") or o.get("save") or o.get("out2"))
        mode = -1 if layer < 0 or not plain else layer + (2 if zero else 0)
        if EXACT:
            name += "/f32"
    else:  # launch_lstm_cfg: the fixed modes take no mask and no row_len, and not the zero-state form
        plain = not (o.get("masks") or o.get("row_len") or zero)
        mode = -1 if layer < 0 or not plain else layer
    return name.format(mode=mode)


def compare(what, got, want, bound):
    """|got - want| <= bound at every element (equality where the bound is 0); returns the worst ratio"""
    got = got.detach().cpu().numpy().astype(np.float64)
    assert got.shape == want.shape == bound.shape, (what, got.shape, want.shape, bound.shape)
    assert np.isfinite(got).all(), "%s: non-finite values" % what
    err = np.abs(got - want)
    exact = bound == 0
    assert not np.any(exact & (err != 0)), "%s: %d elements that must be copies differ (worst %.3g)" % (what, int(np.sum(exact & (err != 0))), err[exact].max())
    ratio = float(np.max(np.where(exact, 0.0, err / np.where(exact, 1.0, bound)))) if got.size else 0.0
    assert ratio <= 1.0, "%s: error / bound %.3f at %s (error %.3g)" % (what, ratio, np.unravel_index(np.argmax(np.where(exact, 0.0, err / np.where(exact, 1.0, bound))), err.shape), err.max())
    return ratio


@pytest.mark.parametrize("cid,opt,live", PARAMS, ids=["%s-%s%s" % (c, o, "-live" if lv else "") for c, o, lv in PARAMS])
def test_lstm_step_vs_float64(lib, cid, opt, live):
    from fcl_taco2_amd import ops

    if EXACT and cid not in EXACT_CHILD:
        pytest.skip("the exact-fp32 process runs the cases of EXACT_CHILD")
    st = family_state(lib, ops, cid)
    inp, dv = st["inp"], st["ops"]
    m, u = inp["m"], inp["u"]
    o = R.OPTIONS[opt]
    m_live = m * 5 // 8 + 1 if live else None  # (not a multiple of 16 for the M of CASES: the last live tile is ragged)
    terms, h_in, c_in, kw = R.option_kwargs(inp, opt, m_dev=m_live)
    zero = h_in is None
    if len(terms) not in st["mm"]:
        if threadpool_limits is None:
            st["mm"][len(terms)] = R.contraction_f64(terms)
        else:
            with threadpool_limits(limits=16):
                st["mm"][len(terms)] = R.contraction_f64(terms)
    ref = R.lstm_step_f64(st["mm"][len(terms)], u, h_in, c_in, **kw)
    bound = R.lstm_step_bound(ref)
    rows = ref["rows"]

    a = lib.LstmStep()
    a.nterms, a.M, a.U = len(terms), m, u
    for i in range(len(terms)):
        a.term[i] = dv.terms[i]
    sd = dv.side
    if o.get("g"):
        a.G, a.g_row_mul, a.g_row_add = sd["g"].data_ptr(), 1, 0
    if o.get("g_t"):
        a.G, a.g_row_mul, a.g_row_add = sd["g_t"].data_ptr(), R.T_BILSTM, R.T_STEP
    if o.get("bias"):
        a.bias = sd["bias"].data_ptr()
    if o.get("pos"):
        a.rank1_w, a.dur = sd["wpos"].data_ptr(), sd["dur"].data_ptr()
    a.step = kw.get("step", 0)
    a.zoneout = kw["zoneout"]
    if o.get("masks"):
        a.zone_keep_h, a.zone_keep_c = sd["keep_h"].data_ptr(), sd["keep_c"].data_ptr()
    if o.get("row_len"):
        a.row_len = sd["row_len"].data_ptr()
    bufs = {}
    bufs["h"] = guarded((m, u), torch.float32, R.SENTINEL)
    bufs["c"] = guarded((m, u), torch.float32, R.SENTINEL)
    if not zero:
        bufs["c"][1].copy_(sd["c_in"])
        a.h_in = sd["h_in"].data_ptr()
    a.h_out, a.c = bufs["h"][1].data_ptr(), bufs["c"][1].data_ptr()
    want_planes = u % 32 == 0 and not EXACT
    if want_planes:
        bufs["hp"] = guarded((m, u // 32 * 64), torch.int16, 0x0707)
        a.h_out_p, a.ld_hp = bufs["hp"][1].data_ptr(), u // 32
    if o.get("save"):
        for k, w in (("gates", 4 * u), ("c_new", u), ("c_old", u), ("h_old", u)):
            bufs[k] = guarded((m, w), torch.float32, R.SENTINEL)
        a.save_gates, a.save_c_new = bufs["gates"][1].data_ptr(), bufs["c_new"][1].data_ptr()
        a.save_c_old, a.save_h_old = bufs["c_old"][1].data_ptr(), bufs["h_old"][1].data_ptr()
    lay = R.out2_layout(inp, opt)
    if lay:
        shape, lkw = lay
        bufs["out2"] = guarded(shape, torch.float32, R.SENTINEL)
        a.out2, a.ld2, a.out2_col_off = bufs["out2"][1].data_ptr(), shape[1], lkw.get("out2_col_off", 0)
        a.out2_row_mul, a.out2_row_add = lkw.get("out2_row_mul", 0), lkw.get("out2_row_add", 0)
        if "out2_row_base" in lkw:
            a.out2_row_base = sd["frame_off"].data_ptr()
    if m_live is not None:
        m_dev = dev(np.array([m_live], np.int32))
        a.m_dev = m_dev.data_ptr()

    lib.prof_enable(True)
    lib.check(lib.load().fcl_lstm_step_fwd(C.byref(a), ops._stream()))
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:  # a device fault: nothing more may start on this GPU
        pytest.exit("%s-%s: the device reported %s" % (cid, opt, e), returncode=3)
    names = sorted(lib.prof_collect())
    lib.prof_enable(False)
    assert names == [expected_kernel(cid, opt, zero)], names

    for k, (full, _) in bufs.items():
        assert guards_intact(full), "%s: a guard line was overwritten" % k
    ratios = {}
    for k in ("h", "c"):
        ratios[k] = compare(k, bufs[k][1][:rows], ref[k][:rows], bound[k][:rows])
    before = {"h": None, "c": None if zero else sd["c_in"][rows:]}
    for k, (_, view) in bufs.items():
        if k in ("out2", "hp"):
            continue
        tail = view[rows:]
        if before.get(k) is not None:
            assert torch.equal(tail, before[k]), "%s: rows past the device's row count changed" % k
        else:
            assert bool((tail == R.SENTINEL).all()), "%s: rows past the device's row count were written" % k
    if o.get("save"):
        ratios["gates"] = compare("save_gates", bufs["gates"][1][:rows], ref["gates"][:rows], bound["gates"][:rows])
        ratios["c_new"] = compare("save_c_new", bufs["c_new"][1][:rows], ref["c_new"][:rows], bound["c_new"][:rows])
        zeros = np.zeros((rows, u))
        compare("save_c_old", bufs["c_old"][1][:rows], ref["c_old"][:rows], zeros)
        compare("save_h_old", bufs["h_old"][1][:rows], ref["h_old"][:rows], zeros)
    if lay:
        prev = np.full(shape, R.SENTINEL)
        want2, _ = R.out2_scatter(prev, ref, **lkw)
        bound2, _ = R.out2_scatter(np.zeros(shape), ref, values=bound["out2"], **lkw)  # (0 wherever the step writes nothing: the sentinel must stay)
        ratios["out2"] = compare("out2", bufs["out2"][1], want2, bound2)
    if want_planes:
        got_p = bufs["hp"][1].cpu().numpy().view(np.uint16).reshape(m, u // 32, 2, 32)
        assert np.array_equal(got_p[:rows], split_planes_np(bufs["h"][1][:rows].cpu().numpy())), "h_out_p is not the split of h_out"
        assert np.all(got_p[rows:] == 0x0707), "h_out_p: rows past the device's row count were written"
    print("RATIO %s %s%s %s delta %.2e %s" % (names[0], cid, "-live" if live else "", opt, bound["delta"],
                                            " ".join("%s %.3f" % kv for kv in sorted(ratios.items()))))


@pytest.mark.skipif(EXACT, reason="already the exact-fp32 process")
def test_exact_fp32_forms_in_a_child_process():
    """FCL_PRECISION=0 is read once per process: a child pytest runs lstm_small_ff_kernel/f32 (M = 17) and plstm_kernel<2,2,1,4,...>/f32 (M = 520) /
    plstm_kernel<2,2,2,3,...>/f32 (M = 600) through test_lstm_step_vs_float64, same reference and bound."""
    n = sum(1 for cid, _, _ in PARAMS if cid in EXACT_CHILD)
    env = dict(os.environ, FCL_PRECISION="0")
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-s", "-k",
           "test_lstm_step_vs_float64 and (%s)" % " or ".join(c + "-" for c in EXACT_CHILD), "-p", "no:cacheprovider"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    print("\n".join(line for line in r.stdout.splitlines() if line.startswith("RATIO")))
    tail = "\n".join((r.stdout + "\n" + r.stderr).strip().splitlines()[-25:])
    assert r.returncode == 0, "the FCL_PRECISION=0 child failed:\n" + tail
    assert "%d passed" % n in r.stdout.strip().splitlines()[-1], tail
