"""-m gpu: the register-resident small LSTM step (U = 256, K = 256 terms: lstm_small_resident_kernel<OpsX3>, and <OpsF32> on fragment-major fp32
weights) with BOTH terms' activation rows in one LDS tile, against the float64 cell of tests/lstm_step_ref.py at its per-element bound.

M = 1, 16, 17, 33 (one row; exactly one tile; one tile plus a row; two tiles plus a row) x option sets l0, l1 (two terms) and l0z, l1z (one term,
h_in == NULL), and M = 17 once more with the device's row count at 11.  The two terms' activations come from different distributions
(tests/small_step_rows_inputs.py; tests/test_small_step_rows_cpu.py shows that a tile read from the wrong half exceeds the bound on these arrays).
As tests/test_gpu_lstm_step_f64.py, every case asserts the launched kernel (from the library's launch record), h and c within the bound, guard lines
of a NaN pattern around every written buffer, and the sentinel in rows from min(M, *m_dev) on.  Under FCL_PRECISION=0 (read once per process) a
child pytest re-runs the M = 17 cases: there the fp32-fragment operands select the fp32 form as well."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import lstm_step_ref as R
import small_step_rows_inputs as S
import test_gpu_lstm_step_f64 as T  # its operand / guard / compare helpers (not its cases)
from helpers import split_planes_np

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = T.EXACT
KINDS = ("ff",) if EXACT else ("frag", "ff")
KERNEL = {"frag": T.SMALL_X3, "ff": T.SMALL_FF}
PARAMS = [(m, kind, opt, None) for m in S.MS for kind in KINDS for opt in S.TWO_TERM + S.ONE_TERM]
PARAMS += [(S.M_LIVE[0], kind, opt, S.M_LIVE[1]) for kind in KINDS for opt in S.TWO_TERM + S.ONE_TERM]

_ops = {}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib

    _lib.load()
    return _lib


@pytest.mark.parametrize("m,kind,opt,m_live", PARAMS, ids=["m%d-%s-%s%s" % (m, k, o, "-live%d" % lv if lv else "") for m, k, o, lv in PARAMS])
def test_small_step_rows_vs_float64(lib, m, kind, opt, m_live):
    from fcl_taco2_amd import ops

    inp = S.inputs(m)
    if (m, kind) not in _ops:
        _ops[(m, kind)] = T.Operands(lib, ops, inp, kind, 0)
    dv = _ops[(m, kind)]
    u = inp["u"]
    o = R.OPTIONS[opt]
    terms, h_in, c_in, kw = R.option_kwargs(inp, opt, m_dev=m_live)
    zero = h_in is None
    ref = R.lstm_step_f64(R.contraction_f64(terms), u, h_in, c_in, **kw)
    bound = R.lstm_step_bound(ref)
    rows = ref["rows"]
    assert rows == (m if m_live is None else m_live)

    a = lib.LstmStep()
    a.nterms, a.M, a.U = len(terms), m, u
    for i in range(len(terms)):
        a.term[i] = dv.terms[i]
    sd = dv.side
    if o.get("g"):
        a.G, a.g_row_mul, a.g_row_add = sd["g"].data_ptr(), 1, 0
    if o.get("bias"):
        a.bias = sd["bias"].data_ptr()
    if o.get("pos"):
        a.rank1_w, a.dur = sd["wpos"].data_ptr(), sd["dur"].data_ptr()
    a.step = kw.get("step", 0)
    a.zoneout = kw["zoneout"]
    bufs = {"h": T.guarded((m, u), torch.float32, R.SENTINEL), "c": T.guarded((m, u), torch.float32, R.SENTINEL)}
    if not zero:
        bufs["c"][1].copy_(sd["c_in"])
        a.h_in = sd["h_in"].data_ptr()
    a.h_out, a.c = bufs["h"][1].data_ptr(), bufs["c"][1].data_ptr()
    if not EXACT:
        bufs["hp"] = T.guarded((m, u // 32 * 64), torch.int16, 0x0707)
        a.h_out_p, a.ld_hp = bufs["hp"][1].data_ptr(), u // 32
    if m_live is not None:
        m_dev = T.dev(np.array([m_live], np.int32))
        a.m_dev = m_dev.data_ptr()

    lib.prof_enable(True)
    lib.check(lib.load().fcl_lstm_step_fwd(C.byref(a), ops._stream()))
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:  # a device fault: nothing more may start on this GPU
        pytest.exit("m%d-%s-%s: the device reported %s" % (m, kind, opt, e), returncode=3)
    names = sorted(lib.prof_collect())
    lib.prof_enable(False)
    assert names == [KERNEL[kind]], names

    for k, (full, _) in bufs.items():
        assert T.guards_intact(full), "%s: a guard line was overwritten" % k
    ratios = {k: T.compare(k, bufs[k][1][:rows], ref[k][:rows], bound[k][:rows]) for k in ("h", "c")}
    assert bool((bufs["h"][1][rows:] == R.SENTINEL).all()), "h: rows past the device's row count were written"
    if zero:
        assert bool((bufs["c"][1][rows:] == R.SENTINEL).all()), "c: rows past the device's row count were written"
    else:
        assert torch.equal(bufs["c"][1][rows:], sd["c_in"][rows:]), "c: rows past the device's row count changed"
    if "hp" in bufs:
        got_p = bufs["hp"][1].cpu().numpy().view(np.uint16).reshape(m, u // 32, 2, 32)
        assert np.array_equal(got_p[:rows], split_planes_np(bufs["h"][1][:rows].cpu().numpy())), "h_out_p is not the split of h_out"
        assert np.all(got_p[rows:] == 0x0707), "h_out_p: rows past the device's row count were written"
    print("RATIO %s m%d%s %s h %.3f c %.3f" % (names[0], m, "-live" if m_live else "", opt, ratios["h"], ratios["c"]))


@pytest.mark.skipif(EXACT, reason="already the exact-fp32 process")
def test_m17_in_an_exact_fp32_child_process():
    """FCL_PRECISION=0 is read once per process: a child pytest re-runs the M = 17 cases (lstm_small_ff_kernel/f32), same reference and bound."""
    n = sum(1 for m, kind, _, _ in PARAMS if m == 17 and kind == "ff")
    env = dict(os.environ, FCL_PRECISION="0")
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-s", "-k", "test_small_step_rows_vs_float64 and m17-",
           "-p", "no:cacheprovider"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    print("\n".join(line for line in r.stdout.splitlines() if line.startswith("RATIO")))
    tail = "\n".join((r.stdout + "\n" + r.stderr).strip().splitlines()[-25:])
    assert r.returncode == 0, "the FCL_PRECISION=0 child failed:\n" + tail
    assert "%d passed" % n in r.stdout.strip().splitlines()[-1], tail
