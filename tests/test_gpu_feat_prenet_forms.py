"""-m gpu: every route of the fused feat/prenet launch (csrc/decoder_step.hip launch_feat_prenet) that the student's shape reaches, through
fcl_decoder_loop_fwd against the oracle's decoder loop -- the cases tests/test_gpu_parity.py::test_decoder_loop_vs_oracle does not reach.

Student hparams (U = P = 256, odim 80), three steps.  `before` and the three taps, at that test's bounds: 1e-4, and test_gpu_parity.py's exact-mode
bound (2e-5) under FCL_PRECISION=0.
  * 4 113 rows, live rows per step 4 113 / 4 097 / 40: steps 0 - 2 launch the register-resident kernel with TWO row tiles per workgroup (4 096 rows and
    up) -- a last workgroup with 17 / one live row, a prenet part (40 rows) far below the feat part (4 097) -- and the trailing feat-only launch
    runs on 40 rows with one row tile per workgroup.
  * 17 rows: a full tile plus a one-row tile (the clamped loads), one row tile per workgroup.
Each in two modes: mask dropout free-running, and no dropout teacher-forced.  The 17 rows once more with the counter-hash dropout and a fixed seed:
finite, and two calls draw the same bits (its statistics: test_gpu_parity.py).
Under FCL_PRECISION=0 (a child pytest: the mode is read once per process) the 17-row cases take the exact register-resident kernels free-running,
and the streaming fp32 feat_prenet_kernel teacher-forced (the exact register-resident form has no teacher input); the launch profile says so.

Written as the safety net of the operand-policy merge of these kernels: it passed on a build of the parent's sources (2026-10-19) before any
kernel changed."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import decoder_case, max_abs, np_state_dict
from fcl_taco2_amd import hparams as HP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = os.environ.get("FCL_PRECISION", "1") == "0"
BOUND = 2e-5 if EXACT else 1e-4
MODES = [(False, True), (True, False)]  # (forced, masked)
MODE_IDS = ["free_mask", "forced_nodrop"]

DUR_RT2 = np.array([3] * 40 + [2] * 4057 + [1] * 16, np.int32)  # live rows per step: 4 113, 4 097, 40
DUR_17 = np.array([3] * 9 + [2] * 5 + [1] * 3, np.int32)        # 17, 14, 9


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from fcl_taco2_amd import _lib

    _lib.load()
    return _lib


def run_case(lib, dur, forced, masked):
    """decoder_case under the launch profile: asserts the bounds, returns the profile's kernel names"""
    from fcl_taco2_amd import ops

    hp = HP.student_hparams() if masked else HP.student_hparams(dropout_rate=0.0)
    lib.prof_enable(True)
    try:
        (before, taps), (ref_before, ref_taps) = decoder_case(ops, hp, len(dur), 11, forced, masked, dur=dur)
        torch.cuda.synchronize()
        prof = lib.prof_collect()
    finally:
        lib.prof_enable(False)
    errs = [max_abs(before, ref_before)] + [max_abs(a, b) for a, b in zip(taps, ref_taps)]
    print("rows %d forced=%s masked=%s: before %.3g  taps %.3g %.3g %.3g" % ((len(dur), forced, masked) + tuple(errs)))
    assert bool(torch.isfinite(before).all()) and float(before.abs().max()) > 0
    assert max(errs) < BOUND, errs
    return prof


@pytest.mark.skipif(EXACT, reason="the two-tile route belongs to the bf16x3 form")
@pytest.mark.parametrize("forced,masked", MODES, ids=MODE_IDS)
def test_two_row_tiles_per_workgroup(lib, forced, masked):
    assert [int((DUR_RT2 > t).sum()) for t in range(3)] == [4113, 4097, 40]
    prof = run_case(lib, DUR_RT2, forced, masked)
    assert prof["feat_prenet_kernel/bf16x3"]["launches"] == 4, sorted(prof)  # three steps + the trailing feat-only launch


@pytest.mark.parametrize("forced,masked", MODES, ids=MODE_IDS)
def test_rows17(lib, forced, masked):
    prof = run_case(lib, DUR_17, forced, masked)
    if not EXACT:
        want = ["feat_prenet_kernel/bf16x3", "lstm_small_kernel/bf16x3"]
    elif forced:
        want = ["feat_prenet_kernel", "lstm_small_ff_kernel/f32"]
    else:
        want = ["feat_prenet_split_kernel/f32", "lstm_small_ff_kernel/f32"]
    for name in want:
        assert name in prof, (name, sorted(prof))
    # three steps + the trailing feat-only launch, which has no teacher input: under FCL_PRECISION=0 it takes the register-resident form
    fp = {k: v["launches"] for k, v in prof.items() if k.startswith("feat_prenet")}
    assert fp == ({"feat_prenet_kernel": 3, "feat_prenet_split_kernel/f32": 1} if EXACT and forced else {want[0]: 4}), fp


@pytest.mark.skipif(EXACT, reason="covered in the default process")
def test_rows17_rng_dropout_is_finite_and_repeatable(lib):
    from fcl_taco2_amd import ops
    from fcl_taco2_amd.plan import SynthesisPlan

    hp = HP.student_hparams()
    plan = SynthesisPlan(np_state_dict(hp), hp, DEV)
    dur, n = DUR_17, len(DUR_17)
    att = torch.from_numpy(np.random.RandomState(17).standard_normal((n, hp.eunits)).astype(np.float32)).to(DEV)
    foff = np.concatenate([[0], np.cumsum(dur)[:-1]]).astype(np.int32)
    live = np.array([(dur > t).sum() for t in range(3)], np.int32)
    outs = []
    for _ in range(2):
        before, taps = ops.decoder_loop(plan.decoder, att, torch.from_numpy(dur).to(DEV), live, torch.from_numpy(foff).to(DEV), int(dur.sum()),
                                        dropout_mode=ops.DROP_RNG, seed=1234, want_taps=True)
        outs.append([before.cpu()] + [t.cpu() for t in taps])
    for a, b in zip(*outs):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    assert float(outs[0][1].abs().max()) > 0 and bool((outs[0][1] == 0).any())  # the prenet tap: some kept, some dropped


@pytest.mark.skipif(EXACT, reason="already the exact-fp32 process")
def test_rows17_in_an_exact_fp32_child_process():
    """FCL_PRECISION=0 is read once per process: a child pytest runs the two 17-row cases under it (routes asserted there from the launch profile)."""
    env = dict(os.environ, FCL_PRECISION="0")
    cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-k", "test_rows17 and (free_mask or forced_nodrop)",
           "-p", "no:cacheprovider"]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    tail = "\n".join((r.stdout + "\n" + r.stderr).strip().splitlines()[-25:])
    assert r.returncode == 0, "the FCL_PRECISION=0 child failed:\n" + tail
    assert "2 passed" in r.stdout.strip().splitlines()[-1], tail
