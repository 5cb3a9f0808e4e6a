"""No GPU: the arrays of tests/test_gpu_small_step_rows.py tell a small LSTM step that reads an activation tile from the wrong half of its LDS tile
from a correct one.  On every (M, two-term option set) of the GPU test, against the float64 statement and its per-element bound (lstm_step_ref):
  * the statement with term 1's rows replaced by term 0's exceeds the bound;
  * the statement with the two terms' rows swapped exceeds the bound;
  * the float32 evaluation of the true statement stays within it (the bound is not so tight that a correct kernel fails).
The one-term (zero-state) forms read one half only; for them the statement evaluated on term 1's rows instead of term 0's must exceed the bound."""
import numpy as np
import pytest

import lstm_step_ref as R
import small_step_rows_inputs as S


def _ref(inp, opt):
    terms, h_in, c_in, kw = R.option_kwargs(inp, opt)
    ref = R.lstm_step_f64(R.contraction_f64(terms), inp["u"], h_in, c_in, **kw)
    return terms, h_in, c_in, kw, ref, R.lstm_step_bound(ref)


def _wrong(inp, terms, h_in, c_in, kw):
    out = R.lstm_step_f64(R.contraction_f64(terms), inp["u"], h_in, c_in, **kw)
    return out["h"], out["c"]


@pytest.mark.parametrize("m", S.MS)
@pytest.mark.parametrize("opt", S.TWO_TERM)
def test_wrong_half_exceeds_the_bound_two_terms(m, opt):
    inp = S.inputs(m)
    terms, h_in, c_in, kw, ref, bound = _ref(inp, opt)
    (a0, w0), (a1, w1) = terms
    assert not np.array_equal(a0, a1)
    same = S.worst_ratio(ref, bound, *_wrong(inp, [(a0, w0), (a0, w1)], h_in, c_in, kw))
    swapped = S.worst_ratio(ref, bound, *_wrong(inp, [(a1, w0), (a0, w1)], h_in, c_in, kw))
    f32 = R.lstm_step_f32(terms, inp["u"], h_in, c_in, **{k: v for k, v in kw.items() if k != "m_dev"})
    true32 = S.worst_ratio(ref, bound, f32["h"], f32["c"])
    print("M %d %s: term 1 := term 0 %.1f, swapped %.1f, float32 %.3f (error / bound)" % (m, opt, same, swapped, true32))
    assert same > 1.0 and swapped > 1.0
    assert true32 <= 1.0


@pytest.mark.parametrize("m", S.MS)
@pytest.mark.parametrize("opt", S.ONE_TERM)
def test_wrong_half_exceeds_the_bound_one_term(m, opt):
    inp = S.inputs(m)
    terms, h_in, c_in, kw, ref, bound = _ref(inp, opt)
    assert len(terms) == 1 and h_in is None
    (a0, w0), a1 = terms[0], inp["terms"][1][0]
    other = S.worst_ratio(ref, bound, *_wrong(inp, [(a1, w0)], None, None, kw))
    f32 = R.lstm_step_f32(terms, inp["u"], None, None, **{k: v for k, v in kw.items() if k != "m_dev"})
    true32 = S.worst_ratio(ref, bound, f32["h"], f32["c"])
    print("M %d %s: term 1's rows %.1f, float32 %.3f (error / bound)" % (m, opt, other, true32))
    assert other > 1.0
    assert true32 <= 1.0
