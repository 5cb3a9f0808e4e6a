"""-m gpu: the forms of one LSTM step (include/fcl_hip.h fcl_lstm_step_t) that the synthesis decoder loop relies on.

1. The ZERO-STATE form (h_in == NULL: previous hidden and cell state are zero, c write-only, the h . W_hh^T term not passed) equals the call with
   explicit zero buffers bit for bit, in every kernel form the decoder loop reaches at step 0 or for small batches; the selected kernel is read from
   the library's launch profile.  Also under FCL_PRECISION=0 (a child pytest: the mode is read once per process).
2. The fixed synthesis modes of the big-tile kernel start their accumulators from the additive operands (G + position, or the bias): against the
   fp32-operand kernel, which does not, at the bounds of test_gpu_planes.py.
3. fcl_decoder_loop_fwd has no fill of its recurrent state: the same pass over a workspace of 0xFF bytes (NaN everywhere) and over a zeroed one
   gives the same finite frames, with host row bounds above the device's live-row counts and across the hand-over into the row-tile kernel.

These claims are kernel against kernel (bit equality, one form against another); tests/test_gpu_lstm_step_f64.py compares every form of the step with
an independent float64 reference."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import bf16_to_f32, max_abs, np_state_dict
from fcl_taco2_amd import hparams as HP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = os.environ.get("FCL_PRECISION", "1") == "0"
U, K = 256, 256
SENTINEL = 7.0


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return t.to(DEV).contiguous()


def rnd(rng, *shape):
    return rng.standard_normal(shape).astype(np.float32)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib

    _lib.load()
    return _lib


class Operand(object):
    """One contraction term's operands in every form a step kernel may read: fp32, P32 planes, fragment-major bf16 planes / fp32."""

    def __init__(self, ops, A, W):
        self.A, self.W = dev(A), dev(W)
        self.Wff = ops.pack_frag_f32(self.W)
        self.Ap = self.Wp = self.Whi = self.Wlo = None
        if not EXACT:  # (the exact-fp32 plans carry no bf16 forms: the small step then takes the fragment-major fp32 kernel)
            self.Ap, self.Wp = ops.pack_planes(self.A), ops.pack_planes(self.W)
            self.Whi, self.Wlo = ops.pack_frag_bf16(self.W)

    def term(self, _lib, planes=True):
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        k = self.A.shape[1]
        return _lib.GemmTerm(p(self.A), p(self.W), k, k, k, 0, p(self.Whi), p(self.Wlo), p(self.Ap) if planes else None, p(self.Wp) if planes else None,
                             (k + 31) // 32, (k + 31) // 32, 0, p(self.Wff))


def run_step(_lib, ops, terms, m, layer0, side, h_in, c, h_out, hp=None, step=0, m_dev=None, planes=True, both=False):
    """One fcl_lstm_step_fwd call; returns the profile names of what it launched."""
    a = _lib.LstmStep()
    a.nterms, a.M, a.U = len(terms), m, U
    for i, t in enumerate(terms):
        a.term[i] = t.term(_lib, planes)
    if layer0 or both:
        a.G, a.g_row_mul, a.rank1_w, a.dur, a.step = side["G"].data_ptr(), 1, side["wpos"].data_ptr(), side["dur"].data_ptr(), step
    if not layer0 or both:
        a.bias = side["bias"].data_ptr()
    a.h_in, a.h_out, a.c, a.zoneout = (None if h_in is None else h_in.data_ptr()), h_out.data_ptr(), c.data_ptr(), 0.1
    if hp is not None:
        a.h_out_p, a.ld_hp = hp.data_ptr(), U // 32
    if m_dev is not None:
        a.m_dev = m_dev.data_ptr()
    _lib.prof_enable(True)
    _lib.check(_lib.load().fcl_lstm_step_fwd(C.byref(a), ops._stream()))
    torch.cuda.synchronize()
    prof = _lib.prof_collect()
    _lib.prof_enable(False)
    return sorted(prof)


def side_inputs(rng, m):
    return dict(G=dev(rnd(rng, m, 4 * U) * np.float32(0.3)), bias=dev(rnd(rng, 4 * U) * np.float32(0.3)), wpos=dev(rnd(rng, 4 * U) * np.float32(0.3)),
                dur=dev(rng.randint(1, 30, size=m).astype(np.int32)))


def expected_kernel(m, mode):
    if m <= 512:
        return "lstm_small_ff_kernel/f32" if EXACT else "lstm_small_kernel/bf16x3"
    tile = {520: "2,2,1,4", 600: "2,2,2,3", 1930: "4,2,2,2"}[m]
    return "plstm_kernel<%s,%d,4>%s" % (tile, mode, "/f32" if EXACT else "")


# the smallest M that selects each kernel form (launch_lstm_planes / lstm_step_is_small) and leaves a ragged last tile; 1930 also with a device
# row count below M (rows from there on are loaded but not stored)
@pytest.mark.parametrize("m,m_live", [(17, None), (520, None), (600, None), (1930, None), (1930, 1000)], ids=["m17", "m520", "m600", "m1930", "m1930_live1000"])
def test_zero_state_form_equals_explicit_zeros(lib, m, m_live):
    from fcl_taco2_amd import ops

    rng = np.random.RandomState(m)
    w_scale = np.float32(1.0 / np.sqrt(2 * K))
    x = Operand(ops, rnd(rng, m, K), rnd(rng, 4 * U, K) * w_scale)
    hz = Operand(ops, np.zeros((m, K), np.float32), rnd(rng, 4 * U, K) * w_scale)  # the parent-style second term: a zero A
    side = side_inputs(rng, m)
    m_dev = None if m_live is None else dev(np.array([m_live], np.int32))
    rows = m if m_live is None else m_live
    want_planes = not EXACT  # (the exact-fp32 big-tile step writes no planes)
    for layer0 in (True, False):
        outs = []
        for zero_state in (True, False):
            h_out = torch.full((m, U), SENTINEL, device=DEV)
            hp = torch.full_like(ops.planes_empty(m, U, DEV), 0x0707) if want_planes else None
            if zero_state:
                c = torch.full((m, U), float("nan"), device=DEV)
                names = run_step(lib, ops, [x], m, layer0, side, None, c, h_out, hp, m_dev=m_dev)
                assert names == [expected_kernel(m, 2 if layer0 else 3)], names
            else:
                c = torch.zeros(m, U, device=DEV)
                names = run_step(lib, ops, [x, hz], m, layer0, side, torch.zeros(m, U, device=DEV), c, h_out, hp, m_dev=m_dev)
                assert names == [expected_kernel(m, 0 if layer0 else 1)], names
            outs.append((h_out, c, hp))
        (h_z, c_z, hp_z), (h_e, c_e, hp_e) = outs
        assert bool(torch.isfinite(h_e[:rows]).all()) and float(h_e[:rows].abs().max()) > 0.01
        assert torch.equal(h_z[:rows], h_e[:rows]) and torch.equal(c_z[:rows], c_e[:rows]), layer0
        if want_planes:
            assert torch.equal(hp_z[:rows], hp_e[:rows]), layer0
        if rows < m:  # beyond the device's row count every output keeps its previous contents
            assert bool((h_z[rows:] == SENTINEL).all()) and bool(torch.isnan(c_z[rows:]).all()) and bool((h_e[rows:] == SENTINEL).all())
            assert bool((c_e[rows:] == 0).all())
            if want_planes:
                assert bool((hp_z[rows:] == 0x0707).all()) and bool((hp_e[rows:] == 0x0707).all())


@pytest.mark.skipif(EXACT, reason="already the exact-fp32 process")
def test_zero_state_form_in_an_exact_fp32_child_process():
    """FCL_PRECISION=0 is read once per process: a child pytest runs the small (fragment-major fp32) and one big-tile (fp32 lines) case under it."""
    env = dict(os.environ, FCL_PRECISION="0")
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-k",
           "test_zero_state_form_equals_explicit_zeros and (m17 or m600)", "-p", "no:cacheprovider"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    tail = "\n".join((r.stdout + "\n" + r.stderr).strip().splitlines()[-25:])
    assert r.returncode == 0, "the FCL_PRECISION=0 child failed:\n" + tail
    assert "2 passed" in r.stdout.strip().splitlines()[-1], tail


def test_seeded_accumulators_vs_the_fp32_operand_kernel(lib):
    """M = 1930 (the two-stage 128-row tile), non-zero state, step 3: h within 2e-5 and c within 5e-5 of the fp32-operand kernel (no plane pointers in
    that call), the h planes within 2^-15 of h -- the bounds of test_gpu_planes.py::test_lstm_step_on_planes_vs_the_fp32_operand_kernels.
    (A generic-mode call, G and bias together, runs the unseeded MODE -1 code, which this form leaves as it was; its pre-activation is not an
    output of the step, so an init-after-sum restatement of it on the host is not expressible and no such sub-case is here.)"""
    from fcl_taco2_amd import ops

    if not ops.planes_enabled():
        pytest.skip("FCL_PRECISION=0 / FCL_PLANES=0: the pre-split operand path is off")
    m = 1930
    rng = np.random.RandomState(m + 1)
    w_scale = np.float32(1.0 / np.sqrt(2 * K))
    h_prev = rnd(rng, m, U) * np.float32(0.5)
    x, hh = Operand(ops, rnd(rng, m, K), rnd(rng, 4 * U, K) * w_scale), Operand(ops, h_prev, rnd(rng, 4 * U, K) * w_scale)
    side = side_inputs(rng, m)
    c_prev = rnd(rng, m, U)
    for layer0 in (True, False):
        outs = []
        for planes in (False, True):
            h_out, c = torch.empty(m, U, device=DEV), dev(c_prev.copy())
            hp = ops.planes_empty(m, U, DEV) if planes else None
            names = run_step(lib, ops, [x, hh], m, layer0, side, dev(h_prev), c, h_out, hp, step=3, planes=planes)
            assert names[0].startswith("plstm_kernel<4,2,2,2,%d," % (0 if layer0 else 1) if planes else "lstm_step_kernel<"), names
            outs.append((h_out.cpu(), c.cpu(), hp))
        (h0, c0, _), (h1, c1, hp) = outs
        dh, dc = max_abs(h1, h0), max_abs(c1, c0)
        print("layer0=%s: |dh| %.3g  |dc| %.3g" % (layer0, dh, dc))
        assert dh < 2e-5 and dc < 5e-5
        raw = hp.cpu().numpy().view(np.uint16).reshape(m, -1, 2, 32)
        val = (bf16_to_f32(raw[:, :, 0, :]).astype(np.float64) + bf16_to_f32(raw[:, :, 1, :]).astype(np.float64)).reshape(m, -1)[:, :U]
        assert np.max(np.abs(val - h1.numpy())) < 2.0 ** -15


def decoder_pass(lib, ops, plan, att, att_p, dur, foff, bounds, live_dev, fill_byte, tail_from):
    """fcl_decoder_loop_fwd on a workspace pre-filled with `fill_byte`; returns `before`."""
    dw = plan.decoder
    n, n_frames = att.shape[0], int(dur.sum().item())
    nbytes = lib.load().fcl_decoder_loop_workspace_bytes(C.byref(dw.struct), n)
    ws = torch.full((nbytes,), fill_byte, device=DEV, dtype=torch.uint8)
    before = torch.full((n_frames, dw.struct.odim), float("nan"), device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    io = lib.DecoderIO(n=n, lmax=len(bounds), att_c=att.data_ptr(), dur=dur.data_ptr(), live_rows_host=bounds.ctypes.data, frame_off=foff.data_ptr(),
                       dropout_mode=ops.DROP_NONE, before=before.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=nbytes,
                       att_c_p=None if att_p is None else att_p.data_ptr(), live_rows=live_dev.data_ptr(), status=status.data_ptr(), tail_from=tail_from)
    lib.check(lib.load().fcl_decoder_loop_fwd(C.byref(dw.struct), C.byref(io), ops._stream()))
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    return before


def test_decoder_loop_reads_no_unwritten_state(lib):
    """The shipped structure (C = P = U = 256, odim 80), 40 rows of durations 3, 2, 2, 1, ... (sorted), dropout off; the host's bounds of steps 1 and 2
    are above the device's live-row counts, so rows are loaded that no step has stored.  A workspace of 0xFF bytes and a zeroed one must give the same
    finite frames -- also when step 2 is handed to the row-tile kernel (tail_from = 2; 5e-6 from the per-step pass, as test_gpu_decoder_tile.py)."""
    from fcl_taco2_amd import ops
    from fcl_taco2_amd.plan import SynthesisPlan

    hp = HP.student_hparams()
    plan = SynthesisPlan(np_state_dict(hp), hp, DEV)
    assert (plan.decoder.struct.c, plan.decoder.struct.p, plan.decoder.struct.u, plan.decoder.struct.odim) == (256, 256, 256, 80)
    rng = np.random.RandomState(40)
    dur_np = np.array([3] * 5 + [2] * 15 + [1] * 20, np.int32)
    live_np = np.array([40, 20, 5, 0], np.int32)      # the device's counts [lmax + 1]
    bounds = np.array([40, 24, 22], np.int32)         # the host's: step 1 loads rows 20 .. 23 and stores none of them, so step 2 (and the tile
    #                                                   kernel's first row tile) loads rows of the ping-pong halves that no step has written
    att = dev(rnd(rng, 40, 256))
    att_p = ops.pack_planes(att) if ops.planes_enabled() else None
    dur, live_dev = dev(dur_np), dev(live_np)
    foff = dev((np.cumsum(dur_np) - dur_np).astype(np.int32))
    res = {}
    for tail in (0, 2):
        for fill in (0xFF, 0x00):
            res[tail, fill] = decoder_pass(lib, ops, plan, att, att_p, dur, foff, bounds, live_dev, fill, tail)
        assert bool(torch.isfinite(res[tail, 0xFF]).all()) and float(res[tail, 0xFF].abs().max()) > 0
        assert torch.equal(res[tail, 0xFF], res[tail, 0x00]), tail
    assert max_abs(res[2, 0xFF], res[0, 0xFF]) < 5e-6
