"""-m gpu: the row-walking form of the fused feat/prenet launch (csrc/decoder_step.hip feat_prenet_walk_kernel) against the one-tile kernel it
replaces, BIT FOR BIT, through fcl_decoder_loop_fwd with student hparams.

The library reads its tunables once per process, so every side is a child process (this file run as a script): one with FCL_FP_WALK_TILES=0
(the walker off), two that force the walker onto every launch of the shape with FCL_FP_WALK_MIN_TILES=1 -- at the default tiles per workgroup and
at FCL_FP_WALK_TILES=3.  Each child runs every case below and saves every output tensor; the tests compare them with torch.equal.

  rows  durations                    live rows per step   what it hits
  33    [3]*9 + [2]*8 + [1]*16       33 / 17 / 9          two full tiles plus a one-row tile; a last workgroup walking a single tile; a prenet
                                                          part (17, 9 rows) smaller than the feat part (33, 17)
  49    [3]*20 + [2]*13 + [1]*16     49 / 33 / 20         four tiles: at three tiles per workgroup one workgroup walks three tiles, one walks one
  16    [2]*16                       16 / 16              exactly one tile: the loop runs once

Each case free-running with mask dropout and teacher-forced without dropout (helpers.decoder_case), and with the counter-hash dropout at a fixed seed
(P32 operands and outputs: att_c_p given, before_p asked for).  Step 0 has no h1 (no feat part) and the trailing launch is feat-only, by construction.
The launch profile names the walker in the forcing children and not in the other."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
WALK = "feat_prenet_walk_kernel/bf16x3"
ONE_TILE = "feat_prenet_kernel/bf16x3"

DURS = {33: [3] * 9 + [2] * 8 + [1] * 16, 49: [3] * 20 + [2] * 13 + [1] * 16, 16: [2] * 16}
MODES = ["free_mask", "forced_nodrop", "rng"]
SIDES = {"off": {"FCL_FP_WALK_TILES": "0"}, "walk": {"FCL_FP_WALK_MIN_TILES": "1"}, "walk3": {"FCL_FP_WALK_MIN_TILES": "1", "FCL_FP_WALK_TILES": "3"}}
NAMES = ("before", "tap_prenet", "tap_lstm0", "tap_lstm1", "before_p")


def child_main(out_path):
    """every case in this process's library configuration -> out_path (.npz): the output tensors and the profile's feat/prenet launch counts"""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    from helpers import decoder_case, np_state_dict
    from fcl_taco2_amd import _lib, hparams as HP, ops
    from fcl_taco2_amd.plan import SynthesisPlan

    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV).contiguous()  # noqa: E731
    out = {}
    _lib.prof_enable(True)
    for n, dur in DURS.items():
        dur = np.array(dur, np.int32)
        assert len(dur) == n
        for mode in MODES:
            if mode == "rng":
                hp = HP.student_hparams()
                plan = SynthesisPlan(np_state_dict(hp), hp, DEV)
                att = d(np.random.RandomState(n).standard_normal((n, hp.eunits)).astype(np.float32))
                foff = np.concatenate([[0], np.cumsum(dur)[:-1]]).astype(np.int32)
                live = np.ascontiguousarray((dur[None, :] > np.arange(int(dur[0]))[:, None]).sum(1).astype(np.int32))
                before, taps, before_p = ops.decoder_loop(plan.decoder, att, d(dur), live, d(foff), int(dur.sum()), dropout_mode=ops.DROP_RNG, seed=1234,
                                                          want_taps=True, att_c_p=ops.pack_planes(att), want_before_p=True)
                tensors = [before.cpu()] + [t.cpu() for t in taps] + [before_p.cpu()]
            else:
                forced = mode == "forced_nodrop"
                hp = HP.student_hparams(dropout_rate=0.0) if forced else HP.student_hparams()
                (before, taps), _ = decoder_case(ops, hp, n, 11, forced, not forced, dur=dur)
                tensors = [before] + list(taps)
            torch.cuda.synchronize()
            for name, t in zip(NAMES, tensors):
                out["%d/%s/%s" % (n, mode, name)] = t.numpy()
    prof = _lib.prof_collect()
    _lib.prof_enable(False)
    for name in (WALK, ONE_TILE):
        out["launches/" + name] = np.int64(prof[name]["launches"] if name in prof else 0)
    np.savez(out_path, **out)


@pytest.fixture(scope="module")
def sides(tmp_path_factory):
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    res = {}
    for side, env in SIDES.items():
        path = str(tmp_path_factory.mktemp("fp_walk") / (side + ".npz"))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=dict(os.environ, **env), cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, "the %s child failed:\n%s" % (side, "\n".join((r.stdout + "\n" + r.stderr).strip().splitlines()[-25:]))
        res[side] = dict(np.load(path))
    return res


def test_launch_profile_names_the_walker_only_where_it_is_forced(sides):
    n_launches = sum(max(d) + 1 for d in DURS.values()) * len(MODES)  # per case: one launch per step + the trailing feat-only launch
    assert (int(sides["off"]["launches/" + WALK]), int(sides["off"]["launches/" + ONE_TILE])) == (0, n_launches)
    for side in ("walk", "walk3"):
        assert (int(sides[side]["launches/" + WALK]), int(sides[side]["launches/" + ONE_TILE])) == (n_launches, 0), side


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("rows,side", [(33, "walk"), (49, "walk3"), (16, "walk"), (33, "walk3"), (49, "walk"), (16, "walk3")])
def test_walker_is_bit_identical_to_the_one_tile_kernel(sides, rows, side, mode):
    names = NAMES if mode == "rng" else NAMES[:4]
    for name in names:
        key = "%d/%s/%s" % (rows, mode, name)
        ref, got = torch.from_numpy(sides["off"][key]), torch.from_numpy(sides[side][key])
        if name != "before_p":  # (planes are raw bf16 bit patterns)
            assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0, key
        assert torch.equal(ref, got), "%s differs (%s): %d of %d elements" % (key, side, int((ref != got).sum()), ref.numel())
    if mode != "forced_nodrop":  # dropout took place: some prenet outputs kept, some dropped
        tap = sides["off"]["%d/%s/tap_prenet" % (rows, mode)]
        assert (tap == 0).any() and (tap != 0).any()


if __name__ == "__main__":
    child_main(sys.argv[1])
