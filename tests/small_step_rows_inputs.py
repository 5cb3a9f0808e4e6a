"""Seeded inputs of the small-step row-tile tests (tests/test_small_step_rows_cpu.py without a GPU, tests/test_gpu_small_step_rows.py on one).

The register-resident small LSTM step (csrc/decoder_step.hip: lstm_small_resident_kernel<OpsX3> / <OpsF32>) keeps the activation rows of both
K = 256 terms side by side in ONE LDS tile: term 0 in columns 0 - 255, term 1 in columns 256 - 511.  A tile read from the wrong half is a wrong
result only if the two terms' rows differ by more than the test's bound, so the two are drawn from different distributions: term 0's rows are
N(0.25, 1), term 1's (the recurrent term: h_in) 0.5 N(0, 1), independent.  Everything else is lstm_step_ref.step_inputs's."""
import numpy as np

import lstm_step_ref as R

U = 256
MS = (1, 16, 17, 33)  # one row; exactly one 16-row tile; one tile plus a row; two tiles plus a row
TWO_TERM, ONE_TERM = ("l0", "l1"), ("l0z", "l1z")
M_LIVE = (17, 11)  # the one device-row-count run: 11 live rows of 17

_cache = {}


def inputs(m):
    if m not in _cache:
        inp = R.step_inputs(m, U, (U, U), seed=88000 + m)
        (a0, w0), (a1, w1) = inp["terms"]
        assert a1 is inp["h_in"]
        inp["terms"] = [(a0 + np.float32(0.25), w0), (a1, w1)]
        _cache[m] = inp
    return _cache[m]


def worst_ratio(ref, bound, got_h, got_c):
    """max over h and c of |got - ref| / bound over the rows the step writes (every bound is positive here: no dead row, no kept element)"""
    rows = ref["rows"]
    out = 0.0
    for k, got in (("h", got_h), ("c", got_c)):
        b = bound[k][:rows]
        assert np.all(b > 0)
        out = max(out, float(np.max(np.abs(np.asarray(got, np.float64)[:rows] - ref[k][:rows]) / b)))
    return out
