#!/usr/bin/env python3
"""SHA-256 of every output of fcl_decoder_loop_fwd over a fixed list of cases -- to compare two builds of the library bit for bit.

    python3 tools/decoder_loop_digest.py > new.txt;  FCL_LIB=/path/to/old/libfcl_hip.so python3 tools/decoder_loop_digest.py > old.txt;  diff old.txt new.txt

(and the same pair under FCL_PRECISION=0).  Cases: the five shapes of tests/test_gpu_parity.py::test_decoder_loop_vs_oracle and the two duration lists
of tests/test_gpu_feat_prenet_forms.py (4 113 rows: two row tiles per workgroup; 17 rows), each free-running and teacher-forced, with DROP_NONE,
DROP_MASK (closed-form masks) and DROP_RNG (seed 1234).  One line per output tensor: case, tensor, digest."""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import fcl_taco2_amd  # noqa: E402,F401
from fcl_taco2_amd import hparams as HP, ops, synthetic as SYN  # noqa: E402
from fcl_taco2_amd.plan import SynthesisPlan  # noqa: E402
from helpers import TINY_S, TINY_T, np_state_dict  # noqa: E402

DEV = "cuda:0"


def poisson_dur(n_rows):
    return np.sort(np.clip(np.random.RandomState(5).poisson(6, n_rows), 1, 30))[::-1].astype(np.int32).copy()


CASES = [("tinyS", TINY_S, poisson_dur(37)), ("tinyT", TINY_T, poisson_dur(5)), ("S300", HP.student_hparams(), poisson_dur(300)),
         ("S97", HP.student_hparams(), poisson_dur(97)), ("T70", HP.teacher_hparams(), poisson_dur(70)),
         ("S4113", HP.student_hparams(), np.array([3] * 40 + [2] * 4057 + [1] * 16, np.int32)),
         ("S17", HP.student_hparams(), np.array([3] * 9 + [2] * 5 + [1] * 3, np.int32))]


def main():
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV).contiguous()  # noqa: E731
    print("# FCL_PRECISION=%s" % os.environ.get("FCL_PRECISION", "1"))
    for tag, hp, dur in CASES:
        plan = SynthesisPlan(np_state_dict(hp), hp, DEV)
        n, lmax = len(dur), int(dur[0])
        rng = np.random.RandomState(n)
        att = d(rng.standard_normal((n, hp.eunits)).astype(np.float32))
        ys = d(rng.standard_normal((n, lmax, hp.odim)).astype(np.float32))
        keep = d(SYN.closed_form_keep_mask((lmax, 2, n, hp.prenet_units), 7))
        foff = d(np.concatenate([[0], np.cumsum(dur)[:-1]]).astype(np.int32))
        live = np.ascontiguousarray((dur[None, :] > np.arange(lmax)[:, None]).sum(1).astype(np.int32))
        for forced in (False, True):
            for mode, mname in ((ops.DROP_NONE, "none"), (ops.DROP_MASK, "mask"), (ops.DROP_RNG, "rng")):
                before, taps = ops.decoder_loop(plan.decoder, att, d(dur), live, foff, int(dur.sum()), teacher_ys=ys if forced else None, dropout_mode=mode,
                                                prenet_keep=keep if mode == ops.DROP_MASK else None, seed=1234, want_taps=True)
                torch.cuda.synchronize()
                for name, t in zip(("before", "tap_prenet", "tap_lstm0", "tap_lstm1"), (before,) + tuple(taps)):
                    a = t.cpu().numpy()
                    assert np.isfinite(a).all(), (tag, name)
                    print("%s forced=%d drop=%s %s %s" % (tag, forced, mname, name, hashlib.sha256(a.tobytes()).hexdigest()))


if __name__ == "__main__":
    main()
