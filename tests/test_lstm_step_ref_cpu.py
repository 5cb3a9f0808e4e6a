"""No GPU: the float64 statement of the LSTM step (tests/lstm_step_ref.py) and its bound, checked on the very inputs that
tests/test_gpu_lstm_step_f64.py runs on the device.

1. Operand-format model: the cell in float32 numpy, and in float64 on operands rounded to what their P32 planes carry, stays within HALF the bound
   at every element -- a condition on the inputs and the bound (it leaves room for correct arithmetic), not on a kernel.
2. The gate floor of the bound is the smallest power of ten that leaves the float32 evaluation a factor 4.
3. Mutations: ten deliberate restatement errors each exceed the bound on the outputs they affect -- the bound is tight enough to see them.
4. What the inputs must exercise (saturated and linear gates, dead rows, masks, durations).
5. torch.nn.LSTMCell in float64 agrees with the statement to 1e-12 on the plain case."""
import numpy as np
import pytest
import torch

import lstm_step_ref as R
from helpers import bf16_rn, bf16_to_f32, plane_round, split_planes_np

OPTS = ("gen", "l0z", "bilstm", "train1")  # between them: every additive operand, both zoneout forms, the zero-state form, dead rows
_cache = {}


def family(name):
    if name not in _cache:
        _cache.clear()  # (one family at a time: the largest holds ~100 MB)
        _cache[name] = R.family_inputs(name)
    return _cache[name]


def reference(inp, opt, terms=None, **override):
    t, h_in, c_in, kw = R.option_kwargs(inp, opt)
    kw.update(override)
    h_in, c_in = kw.pop("h_in", h_in), kw.pop("c_in", c_in)
    ref = R.lstm_step_f64(R.contraction_f64(t if terms is None else terms), inp["u"], h_in, c_in, **kw)
    return ref, R.lstm_step_bound(ref)


def plane_value(x):
    """float32 [R, K] -> the float64 value its P32 planes carry (helpers.split_planes_np: hi + lo)"""
    p = split_planes_np(np.ascontiguousarray(x))
    v = bf16_to_f32(p[:, :, 0, :]).astype(np.float64) + bf16_to_f32(p[:, :, 1, :]).astype(np.float64)
    return v.reshape(x.shape[0], -1)[:, : x.shape[1]]


def worst_share(got, ref, bound, keys=("gates", "c_new", "h", "c")):
    """max over outputs and elements of |got - ref| / bound (an element of bound 0 must match exactly)"""
    worst = 0.0
    for k in keys:
        err, b = np.abs(np.asarray(got[k], np.float64) - ref[k]), bound[k]
        assert not np.any((b == 0) & (err != 0)), k
        worst = max(worst, float(np.max(np.where(b > 0, err / np.where(b > 0, b, 1.0), 0.0))))
    return worst


def model_shares(name, opt, floor=R.GATE_FLOOR):
    inp = family(name)
    terms, h_in, c_in, kw = R.option_kwargs(inp, opt)
    ref = R.lstm_step_f64(R.contraction_f64(terms), inp["u"], h_in, c_in, **kw)
    bound = R.lstm_step_bound(ref, floor)
    f32 = R.lstm_step_f32(terms, inp["u"], h_in, c_in, **kw)
    rounded = R.lstm_step_f64(R.contraction_f64([(plane_value(a), plane_value(w)) for a, w in terms]), inp["u"], h_in, c_in, **kw)
    return worst_share(f32, ref, bound), worst_share(rounded, ref, bound), bound


@pytest.mark.parametrize("name", sorted(R.FAMILIES))
def test_operand_format_models_stay_within_half_the_bound(name):
    for opt in OPTS:
        s32, spl, bound = model_shares(name, opt)
        print("%s/%s: float32 %.3f  plane-rounded %.3f of the bound; max bound h %.2e c %.2e" % (name, opt, s32, spl, bound["h"].max(), bound["c"].max()))
        assert s32 <= 0.5 and spl <= 0.5, (name, opt, s32, spl)


def test_plane_value_is_plane_round():
    x = np.random.RandomState(5).standard_normal((7, 45)).astype(np.float32)
    assert np.array_equal(plane_value(x), plane_round(torch.from_numpy(x).double()).numpy())


def test_gate_floor_is_the_smallest_power_of_ten():
    """With a factor 4 to spare at GATE_FLOOR on every family; at a tenth of it, not."""
    worst = {R.GATE_FLOOR: 0.0, R.GATE_FLOOR / 10: 0.0}
    for name in ("m17", "u24_m17", "u32_m70", "wide_m65", "m520", "t3_m513"):
        for opt in OPTS:
            for fl in worst:
                worst[fl] = max(worst[fl], model_shares(name, opt, fl)[0])
    print("float32 share of the bound: %s" % worst)
    assert worst[R.GATE_FLOOR] <= 0.25 < worst[R.GATE_FLOOR / 10]


def exceeds(mut, ref, bound, key):
    return bool(np.any(np.abs(np.asarray(mut, np.float64) - ref[key]) > bound[key]))


def swap_if(x, u):
    """gate blocks i and f exchanged along the last axis"""
    x = np.array(x)
    x[..., :u], x[..., u: 2 * u] = np.array(x[..., u: 2 * u]), np.array(x[..., :u])
    return x


@pytest.mark.parametrize("name", ["m17", "u24_m17"])
def test_mutations_exceed_the_bound(name):
    inp = family(name)
    u = inp["u"]

    # 1. i / f gate order swapped: the kernel would read gate block 1 as i and block 0 as f
    ref, bound = reference(inp, "gen")
    terms = [(a, swap_if(w.T, u).T) for a, w in inp["terms"]]
    mut, _ = reference(inp, "gen", terms=terms, g=swap_if(inp["g"], u), bias=swap_if(inp["bias"], u), rank1_w=swap_if(inp["wpos"], u))
    assert exceeds(mut["h"], ref, bound, "h") and exceeds(mut["c"], ref, bound, "c") and exceeds(mut["gates"], ref, bound, "gates")

    # 2. zoneout blend direction swapped: (1 - rate) * old + rate * new
    mut, _ = reference(inp, "gen", zoneout=1.0 - R.ZONEOUT)
    assert exceeds(mut["h"], ref, bound, "h") and exceeds(mut["c"], ref, bound, "c")

    # 4. position (step + 1) / dur
    mut, _ = reference(inp, "gen", step=R.STEP + 1)
    assert exceeds(mut["h"], ref, bound, "h") and exceeds(mut["c"], ref, bound, "c")

    # 6. the lo plane of one operand dropped (a bf16 x 2 product): the first term's activations at their hi plane alone
    a0, w0 = inp["terms"][0]
    mut, _ = reference(inp, "gen", terms=[(bf16_to_f32(bf16_rn(a0)), w0)] + list(inp["terms"][1:]))
    assert exceeds(mut["h"], ref, bound, "h") and exceeds(mut["c"], ref, bound, "c")

    # 7. c_old taken as 0 on a non-zero-state step
    mut, _ = reference(inp, "gen", c_in=np.zeros_like(inp["c_in"]))
    assert exceeds(mut["h"], ref, bound, "h") and exceeds(mut["c"], ref, bound, "c")

    # 3. mask polarity inverted (training form) and 10. save_c_new taken after zoneout
    ref, bound = reference(inp, "train1")
    mut, _ = reference(inp, "train1", zone_keep_h=1 - inp["keep_h"], zone_keep_c=1 - inp["keep_c"])
    assert exceeds(mut["h"], ref, bound, "h") and exceeds(mut["c"], ref, bound, "c")
    assert not exceeds(mut["c_new"], ref, bound, "c_new")  # (the raw cell does not depend on the masks)
    assert exceeds(ref["c"], ref, bound, "c_new")

    # 5. G row off by one, 8. a dead row updated, 9. out2 written one row off (BiLSTM form)
    ref, bound = reference(inp, "bilstm")
    for d in (-1, 1):
        mut, _ = reference(inp, "bilstm", g_row_add=R.T_STEP + d)
        assert exceeds(mut["h"], ref, bound, "h") and exceeds(mut["c"], ref, bound, "c"), d
    mut, _ = reference(inp, "bilstm", row_len=None)
    dead = ~ref["live"]
    assert dead.any() and exceeds(mut["h"][dead], {"h": ref["h"][dead]}, {"h": bound["h"][dead]}, "h")
    assert exceeds(mut["c"][dead], {"c": ref["c"][dead]}, {"c": bound["c"][dead]}, "c")
    shape, lay = R.out2_layout(inp, "bilstm")
    prev = np.full(shape, R.SENTINEL)
    want, written = R.out2_scatter(prev, ref, **lay)
    b2 = R.out2_scatter(np.zeros(shape), ref, values=bound["out2"], **lay)[0]
    assert written.sum() == inp["m"] * u and np.all(want[~written] == R.SENTINEL)
    assert np.all(want[written].reshape(inp["m"], u)[dead] == 0.0)  # a dead row's tap is 0, not its passed-through state
    off = R.out2_scatter(prev, ref, **dict(lay, out2_row_add=lay["out2_row_add"] + 1))[0]
    assert np.any(np.abs(off - want) > b2)
    # ... and a dead row's tap written as its state instead of 0
    leak = R.out2_scatter(prev, ref, values=ref["h"], **lay)[0]
    assert np.any(np.abs(leak - want) > b2)


@pytest.mark.parametrize("name", sorted(R.FAMILIES))
def test_input_conditions(name):
    """Gate pre-activations of the generic form: at least 10 % in the linear region (|pre| < 1) and at least 2 % saturated (|pre| > 4: sigmoid'
    < 0.018, 1 - tanh^2 < 0.0014), in every gate; the contraction part alone has rms 0.25 .. 0.75 (at or below the unit scale the GEMM bound is stated at)."""
    inp = family(name)
    m, u = inp["m"], inp["u"]
    ref, _ = reference(inp, "gen")
    rms = float(np.sqrt(np.mean(ref["mm"] ** 2)))
    assert 0.25 < rms < 0.75, rms
    for gate in range(4):
        p = np.abs(ref["pre"][:, gate * u: (gate + 1) * u])
        lin, sat = float(np.mean(p < 1.0)), float(np.mean(p > 4.0))
        assert lin >= 0.10 and sat >= 0.02, (name, gate, lin, sat)
    assert inp["dur"].min() >= 1 and inp["dur"].dtype == np.int32
    assert np.all(np.diff(inp["frame_off"]) >= 1) and inp["frame_off"][0] == 0
    if m >= 3:  # dead rows at t = T_STEP, one of them of length 0, beside live ones
        dead = ~(R.T_STEP < inp["row_len"])
        assert dead.any() and (~dead).any() and (inp["row_len"] == 0).any()
    if m * u >= 256:
        for k in ("keep_h", "keep_c"):
            assert 0.4 < inp[k].mean() < 0.6 and set(np.unique(inp[k])) == {0, 1}
        assert 0.4 < np.mean(inp["keep_h"] != inp["keep_c"]) < 0.6  # independent masks
    for a, w in inp["terms"]:
        assert a.dtype == np.float32 and w.dtype == np.float32 and a.shape[0] == m and w.shape[0] == 4 * u


def test_agrees_with_torch_lstmcell_in_float64():
    inp = family("m17")
    u = inp["u"]
    (x, w_ih), (hh, w_hh) = inp["terms"]
    assert hh is inp["h_in"]
    cell = torch.nn.LSTMCell(x.shape[1], u).double()
    with torch.no_grad():
        cell.weight_ih.copy_(torch.from_numpy(w_ih).double())
        cell.weight_hh.copy_(torch.from_numpy(w_hh).double())
        cell.bias_ih.copy_(torch.from_numpy(inp["bias"]).double())
        cell.bias_hh.zero_()
        h, c = cell(torch.from_numpy(x).double(), (torch.from_numpy(hh).double(), torch.from_numpy(inp["c_in"]).double()))
    ref = R.lstm_step_f64(R.contraction_f64(inp["terms"]), u, hh, inp["c_in"], bias=inp["bias"])
    assert np.max(np.abs(ref["h"] - h.numpy())) < 1e-12 and np.max(np.abs(ref["c"] - c.numpy())) < 1e-12
    assert np.array_equal(ref["h"], ref["h_new"]) and np.array_equal(ref["c"], ref["c_new"])  # no zoneout, every row live
