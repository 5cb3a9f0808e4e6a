"""No GPU: the float64 statements of the training step's element-wise and reduction operations (tests/train_pointwise_ref.py) and their bounds,
checked on the very inputs that tests/test_gpu_train_pointwise_f64.py runs on the device.

(a) Every statement agrees with torch in float64 on the CPU to 1e-10: F.batch_norm(training=True) with running buffers and its autograd (bn_stats,
    bn_act, bn_bwd, colsum modes 0 and 3 as dbeta and dgamma), F.layer_norm + dropout mask + head + masked_fill and its autograd, F.conv1d(1 -> C, k)
    per segment, F.normalize.  torch refuses M = 1 in train mode: that case is checked against the written formula.
(b) The float32 numpy evaluation of each expression in the kernel's order of operations (R.f32_*) uses at most HALF of its bound at every element
    of every case -- a condition on the inputs and the bounds (it leaves room for correct arithmetic), not on a kernel; and the bn_act expression
    uses more than half of a 2^-22 bound at (131, 132), which is why that bound is 2^-21.  One expression cannot meet one half: the sigmoid
    backward g * (y * (1 - y)) is 2.5 roundings against a bound of 4 (0.515 on the 33 x 96 inputs); it is held to its derived worst case 0.625.
(c) The case tables select the kernel forms they claim: C % 4, the operand offset of the scalar twin, the M >= 8192 threshold, ragged column groups,
    the LayerNorm arms and the rows-per-wave of its backward."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_pointwise_ref as R

T64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))  # noqa: E731
ACT_T = {R.ACT_NONE: lambda v: v, R.ACT_RELU: torch.relu, R.ACT_TANH: torch.tanh, R.ACT_SIGMOID: torch.sigmoid}


def agree(what, got, want, tol=1e-10):
    got, want = np.asarray(got, np.float64), want.detach().numpy() if hasattr(want, "detach") else np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    worst = float(np.max(np.abs(got - want) / (1.0 + np.abs(want)))) if got.size else 0.0
    assert worst <= tol, "%s: differs from torch by %.3g" % (what, worst)


def used(what, got, want, bound, limit=0.5):
    """worst |got - want| / bound; elements with bound 0 must be equal"""
    got, want, bound = np.asarray(got, np.float64), np.asarray(want, np.float64), np.broadcast_to(np.asarray(bound, np.float64), np.shape(want))
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err, exact = np.abs(got - want), bound == 0
    assert not np.any(exact & (err != 0)), "%s: %d elements that must be exact differ" % (what, int(np.sum(exact & (err != 0))))
    ratio = float(np.max(np.where(exact, 0.0, err / np.where(exact, 1.0, bound)))) if got.size else 0.0
    assert ratio <= limit, "%s: the float32 evaluation uses %.3f of the bound" % (what, ratio)
    return ratio


# ---- bn_stats ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", sorted(R.BN_STATS_CASES))
def test_bn_stats(cid):
    d = R.bn_stats_inputs(cid)
    m, c, mom = d["m"], d["c"], d["momentum"]
    ref = R.ref_bn_stats(d["z"], R.BN_EPS, mom, d["running_mean"], d["running_var"])
    eps = R.wide(R.BN_EPS)
    assert ref["var"][d["const_col"]] == 0.0 and ref["invstd"][d["const_col"]] == 1.0 / np.sqrt(eps)
    if m == 1:  # the written formula: var = 0, the unbiased variance is var itself
        w = R.wide(mom)
        assert np.array_equal(ref["mean"], d["z"][0].astype(np.float64)) and np.all(ref["var"] == 0)
        agree("running_mean", ref["running_mean"], (1 - w) * d["running_mean"].astype(np.float64) + w * d["z"][0].astype(np.float64))
        agree("running_var", ref["running_var"], (1 - w) * d["running_var"].astype(np.float64))
    else:
        rm = None if d["running_mean"] is None else T64(d["running_mean"]).clone()
        rv = None if d["running_var"] is None else T64(d["running_var"]).clone()
        y = F.batch_norm(T64(d["z"]), rm, rv, None, None, True, R.wide(mom), eps)
        one, zero = np.ones(c), np.zeros(c)
        agree("normalised z", R.ref_bn_act(d["z"], ref["mean"], ref["invstd"], one, zero, R.ACT_NONE)["y_act"], y)
        if rm is not None:
            agree("running_mean", ref["running_mean"], rm)
            agree("running_var", ref["running_var"], rv)
    got = R.f32_bn_stats(d["z"], R.BN_EPS, mom, d["running_mean"], d["running_var"])
    bound = R.bound_bn_stats(d["z"], ref, mom, d["running_mean"])
    for k in bound:
        used("bn_stats %s %s" % (cid, k), got[k], ref[k], bound[k])


# ---- bn_act / bn_bwd / colsum as dbeta, dgamma -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,c", R.BN_SHAPES)
def test_bn_act_and_bwd(m, c):
    d = R.bn_inputs(m, c)
    st = R.ref_bn_stats(d["z"])  # the unrounded statistics: what torch normalises with
    eps = R.wide(R.BN_EPS)
    keep_t = T64(d["keep"])
    for act in R.BN_ACTS:
        z = T64(d["z"]).requires_grad_(True)
        g, b = T64(d["gamma"]).requires_grad_(True), T64(d["beta"]).requires_grad_(True)
        y = F.batch_norm(z, None, None, g, b, True, 0.1, eps)
        ya = ACT_T[act](y)
        ref = R.ref_bn_act(d["z"], st["mean"], st["invstd"], d["gamma"], d["beta"], act, d["keep"], R.KEEP_SCALE)
        agree("y_act", ref["y_act"], ya)
        agree("y_drop", ref["y_drop"], ya * keep_t * R.KEEP_SCALE)
        if act == R.ACT_NONE:
            (y * T64(d["dy"])).sum().backward()
            dbeta, dgamma = b.grad.numpy(), g.grad.numpy()
            agree("dbeta = colsum mode 0", R.ref_colsum(R.colsum_terms(d["dy"]), np.zeros(c)), dbeta)
            agree("dgamma = colsum mode 3", R.ref_colsum(R.colsum_terms(d["dy"], d["z"], st["invstd"], st["mean"], 3), np.zeros(c)), dgamma)
            agree("dz", R.ref_bn_bwd(d["dy"], d["z"], st["mean"], st["invstd"], d["gamma"], dbeta, dgamma)["dz"], z.grad)
        # the float32 model on the inputs the kernel receives
        for keep in (None, d["keep"]):
            ks = 1.0 if keep is None else R.KEEP_SCALE
            ref = R.ref_bn_act(d["z"], d["mean"], d["invstd"], d["gamma"], d["beta"], act, keep, ks)
            bound = R.bound_bn_act(ref, d["gamma"], d["beta"], act, keep, ks)
            got = R.f32_bn_act(d["z"], d["mean"], d["invstd"], d["gamma"], d["beta"], act, keep, ks)
            used("bn_act y_act", got["y_act"], ref["y_act"], bound["y_act"])
            used("bn_act y_drop", got["y_drop"], ref["y_drop"], bound["y_drop"])
            if keep is not None:
                assert np.all(got["y_drop"][keep == 0] == 0) and np.array_equal(got["y_drop"][keep != 0], 2 * got["y_act"][keep != 0])
    ref = R.ref_bn_bwd(d["dy"], d["z"], d["mean"], d["invstd"], d["gamma"], d["dbeta"], d["dgamma"], acc=(d["acc_dbeta"], d["acc_dgamma"]))
    used("bn_bwd dz", R.f32_bn_bwd(d["dy"], d["z"], d["mean"], d["invstd"], d["gamma"], d["dbeta"], d["dgamma"]), ref["dz"],
         R.bound_bn_bwd(ref, d["dy"], d["invstd"], d["gamma"], d["dbeta"], d["dgamma"]))
    assert ref["acc_dbeta"].dtype == np.float32 and np.array_equal(ref["acc_dbeta"], d["acc_dbeta"] + d["dbeta"])


def test_bn_bounds_are_tight():
    """at (131, 132) the float32 expressions use well under half of the 2^-21 bounds, and bn_act more than half of a 2^-22 one"""
    d = R.bn_inputs(131, 132)
    ref = R.ref_bn_act(d["z"], d["mean"], d["invstd"], d["gamma"], d["beta"], R.ACT_NONE)
    r_act = used("bn_act", R.f32_bn_act(d["z"], d["mean"], d["invstd"], d["gamma"], d["beta"], R.ACT_NONE)["y_act"], ref["y_act"],
                 R.bound_bn_act(ref, d["gamma"], d["beta"], R.ACT_NONE)["y_act"])
    rb = R.ref_bn_bwd(d["dy"], d["z"], d["mean"], d["invstd"], d["gamma"], d["dbeta"], d["dgamma"])
    r_bwd = used("bn_bwd", R.f32_bn_bwd(d["dy"], d["z"], d["mean"], d["invstd"], d["gamma"], d["dbeta"], d["dgamma"]), rb["dz"],
                 R.bound_bn_bwd(rb, d["dy"], d["invstd"], d["gamma"], d["dbeta"], d["dgamma"]))
    print("bn_act %.3f bn_bwd %.3f of the 2^-21 bounds" % (r_act, r_bwd))
    assert r_act > 0.25, "bn_act would fit half of a 2^-22 bound (%.3f of 2^-21)" % r_act


# ---- activation maps -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,c", R.ACT_SHAPES)
def test_act_fwd_bwd(r, c):
    d = R.act_inputs(r, c)
    for act in R.ACTS:
        for keep in (None, d["keep"]):
            ks = 1.0 if keep is None else R.KEEP_SCALE
            kf = 1.0 if keep is None else T64(keep) * ks
            x = T64(d["x"]).requires_grad_(True)
            out = ACT_T[act](x) * kf
            ref = R.ref_act_fwd(d["x"], act, keep, ks)
            agree("act_fwd", ref, out)
            used("act_fwd %d" % act, R.f32_act_fwd(d["x"], act, keep, ks), ref, R.bound_act_fwd(ref, act, keep, ks))
            # backward from the saved activation: autograd through the float64 activation of the float32-rounded y's pre-image is not available, so
            # the derivative is taken at y itself -- act'(x) written in y, the form the kernel is handed
            y = T64(d["y"][act])
            dact = {R.ACT_NONE: torch.ones_like(y), R.ACT_RELU: (y > 0).double(), R.ACT_TANH: 1 - y * y, R.ACT_SIGMOID: y * (1 - y)}[act]
            refb = R.ref_act_bwd(d["dy"], d["y"][act], act, keep, ks)
            agree("act_bwd", refb, T64(d["dy"]) * kf * dact)
            used("act_bwd %d" % act, R.f32_act_bwd(d["dy"], d["y"][act], act, keep, ks), refb, R.bound_act_bwd(refb),
                 limit=R.ACT_BWD_SIGMOID_SHARE if act == R.ACT_SIGMOID else 0.5)
            if keep is None:  # and that form is autograd's derivative at x (to the rounding of y: 2^-24 relative on y)
                out.backward(T64(d["dy"]))
                assert float((x.grad - T64(refb)).abs().max()) < 1e-6


# ---- colsum ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,c", R.COLSUM_SHAPES)
def test_colsum(m, c):
    d = R.colsum_inputs(m, c)
    x, y, g, b = (T64(d[k]) for k in ("x", "y", "g", "b"))
    want = {0: x.sum(0), 1: (x * y).sum(0), 2: (x * (y - b) / g).sum(0), 3: (x * (y - b) * g).sum(0)}
    for mode in range(4):
        terms = R.colsum_terms(d["x"], d["y"], d["g"], d["b"], mode)
        ref = R.ref_colsum(terms, d["out"])
        agree("colsum mode %d" % mode, ref, T64(d["out"]) + want[mode])
        used("colsum mode %d" % mode, R.f32_colsum(d["x"], d["y"], d["g"], d["b"], mode, d["out"]), ref, R.bound_colsum(terms, d["out"]))
    tx = R.colsum_terms(d["x"])
    used("colsum out_x", R.f32_colsum(d["x"], None, None, None, 0, d["out_x"]), R.ref_colsum(tx, d["out_x"]), R.bound_colsum(tx, d["out_x"]))


# ---- conv1d_in1_dw ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,c,k,ldy,full", R.CONV_DW_CASES)
def test_conv1d_in1_dw(m, c, k, ldy, full):
    d = R.conv_dw_inputs(m, c, k, ldy, full)
    dy = d["dy_buf"][:, :c]
    assert np.isfinite(dy).all() and (ldy == c or np.isnan(d["dy_buf"][:, c:]).all())
    db0 = d["db"] if full else np.zeros(c, np.float32)
    ref = R.ref_conv1d_in1_dw(dy, d["x"], k, d["dw"][:, 0, :], db0, d["seg_lo"], d["seg_hi"])
    w = torch.zeros(c, 1, k, dtype=torch.float64, requires_grad=True)
    bias = torch.zeros(c, dtype=torch.float64, requires_grad=True)
    lens = R.seg_lens(m) if full else [m]
    off = np.concatenate([[0], np.cumsum(lens)])
    xt = T64(d["x"])
    out = torch.cat([F.conv1d(xt[s:e].reshape(1, 1, -1), w, bias, 1, (k - 1) // 2)[0].t() for s, e in zip(off[:-1], off[1:])])
    (out * T64(dy)).sum().backward()
    agree("dw", ref["dw"], T64(d["dw"][:, 0, :]) + w.grad[:, 0, :])
    agree("db", ref["db"], T64(db0) + bias.grad)
    gw, gb = R.f32_conv1d_in1_dw(dy, d["x"], k, d["dw"][:, 0, :], db0, d["seg_lo"], d["seg_hi"])
    used("conv1d_in1_dw dw", gw, ref["dw"], ref["bound_dw"])
    used("conv1d_in1_dw db", gb, ref["db"], ref["bound_db"])


# ---- unpack, concat --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cout,cin,k", R.UNPACK_SHAPES)
def test_unpack(cout, cin, k):
    d = R.unpack_inputs(cout, cin, k)
    for scale in (None, d["scale"]):
        ref, bound = R.ref_unpack(d["dwp"], d["dw"], scale)
        s = torch.ones(cout, dtype=torch.float64) if scale is None else T64(scale)
        agree("unpack", ref, T64(d["dw"]) + T64(d["dwp"]).permute(1, 2, 0) * s[:, None, None])
        used("unpack", R.f32_unpack(d["dwp"], d["dw"], scale), ref, bound)


@pytest.mark.parametrize("case", R.CONCAT_CASES, ids=lambda cs: "c%d_s%d" % (cs[2], cs[3]))
def test_concat_spk(case):
    b, t, c, s, m, ldh, planes, kinds = case
    d = R.concat_inputs(*case)
    hs = d["hs_buf"][:, :c]
    ref, bound = R.ref_concat_spk(hs, d["spk"], t)
    agree("concat", ref, torch.cat([T64(hs), F.normalize(T64(d["spk"]), dim=1)[torch.arange(m) // t]], 1))
    got = R.f32_concat_spk(hs, d["spk"], t)
    used("concat_spk", got, ref, bound)
    norms = np.sqrt((d["spk"].astype(np.float64) ** 2).sum(1))
    for i, kind in enumerate(kinds):  # the rows are what their names say
        assert {"unit": 1 < norms[i] < 10, "large": norms[i] > 1e3, "tiny": 0 < norms[i] < 1e-12, "zero": norms[i] == 0}[kind], (kind, norms[i])
        if i * t < m and kind == "zero":
            assert np.all(ref[i * t, c:] == 0) and np.all(got[i * t, c:] == 0)


# ---- LayerNorm -------------------------------------------------------------------------------------------------------------------------------------
def torch_ln(d, c, with_dy=True, with_ds=True):
    x, g, b, lw, lb = (T64(d[k]).requires_grad_(True) for k in ("x", "gamma", "beta", "lin_w", "lin_b"))
    y = F.layer_norm(x, (c,), g, b, R.wide(R.LN_EPS)) * T64(d["keep"]) * R.KEEP_SCALE
    s = (y @ lw + lb).masked_fill(torch.from_numpy(d["pad"]).bool(), 0.0)
    loss = (y * T64(d["dy"])).sum() * (1.0 if with_dy else 0.0) + (s * T64(d["ds"])).sum() * (1.0 if with_ds else 0.0)
    loss.backward()
    return y, s, dict(dx=x.grad, dgamma=g.grad, dbeta=b.grad, dlin_w=lw.grad, dlin_b=lb.grad)


@pytest.mark.parametrize("m,c", R.LN_FWD_CASES)
def test_layernorm_fwd(m, c):
    d = R.ln_inputs(m, c)
    y, s, _ = torch_ln(d, c)
    ref = R.ref_layernorm(d["x"], d["gamma"], d["beta"], R.LN_EPS, d["keep"], R.KEEP_SCALE, d["lin_w"], d["lin_b"], d["pad"])
    agree("y", ref["y"], y)
    agree("scalar", ref["scalar"], s)
    got = R.f32_layernorm(d["x"], d["gamma"], d["beta"], R.LN_EPS, d["keep"], R.KEEP_SCALE, d["lin_w"], d["lin_b"], d["pad"])
    used("layernorm y", got["y"], ref["y"], ref["tol_y"])
    used("layernorm scalar", got["scalar"], ref["scalar"], ref["tol_s"])
    assert np.all(ref["tol_y"][d["keep"] == 0] == 0) and np.all(ref["tol_s"][d["pad"] != 0] == 0)


@pytest.mark.parametrize("m,c,with_dy,with_ds", R.LN_BWD_CASES)
def test_layernorm_bwd(m, c, with_dy, with_ds):
    d = R.ln_inputs(m, c)
    _, _, grads = torch_ln(d, c, with_dy, with_ds)
    kw = dict(dy=d["dy"] if with_dy else None, lin_w=d["lin_w"] if with_ds else None, ds=d["ds"] if with_ds else None, pad=d["pad"], keep=d["keep"],
              keep_scale=R.KEEP_SCALE, before=d["before"])
    ref = R.ref_layernorm_bwd(d["x"], d["gamma"], d["beta"], R.LN_EPS, **kw)
    got = R.f32_layernorm_bwd(d["x"], d["gamma"], d["beta"], R.LN_EPS, **kw)
    agree("dx", ref["dx"], grads["dx"])
    assert np.all(ref["dx"][1] == 0) and np.all(ref["bound_dx"][1] == 0), "the row dropped whole passes no gradient"
    used("layernorm_bwd dx", got["dx"], ref["dx"], ref["bound_dx"])
    for k in ("dgamma", "dbeta") + (("dlin_w", "dlin_b") if with_ds else ()):
        agree(k, ref[k] - d["before"][k].astype(np.float64), grads[k])
        used("layernorm_bwd " + k, got[k], ref[k], ref["bound_" + k])


# ---- (c) the cases select the forms they claim --------------------------------------------------------------------------------------------------------
def test_cases_select_their_forms():
    assert [c % 4 != 0 for _, c in R.BN_SHAPES] == [True, True, False, False], "two scalar, two four-wide BatchNorm shapes"
    assert [c for _, c in R.BN_SHAPES if c % 32 == 0] == [96], "planes at C = 96"
    assert (4 * R.TWIN_OFFSET) % 16 != 0, "the twin's operand views must miss 16-byte alignment"
    assert [(r * c) % 4 for r, c in R.ACT_SHAPES] == [3, 0] and R.ACT_SHAPES[1][1] % 32 == 0
    assert [m >= 8192 for m, _ in R.COLSUM_SHAPES] == [False, False, False, True]
    assert [R.rows_per_block(m) for m in (1, 8191, 8192, 8193)] == [64, 64, 128, 128]
    assert sum(m >= 8192 for m, _, _, _ in R.BN_STATS_CASES.values()) == 1
    assert any(c % 64 for _, c in R.COLSUM_SHAPES[1:]) and any(c > 64 and c % 64 for _, c, _, _ in R.BN_STATS_CASES.values()), "a ragged last column group"
    assert {mom for _, _, mom, _ in R.BN_STATS_CASES.values()} == {0.1, 1.0} and sum(not run for _, _, _, run in R.BN_STATS_CASES.values()) == 1
    d = R.bn_stats_inputs("m65_c130")
    assert set(d["off"]) == {0.0, 3.0, 100.0}
    assert [c % 64 != 0 for _, c, _, _, _ in R.CONV_DW_CASES] == [True, True, True, False] and R.CONV_DW_CASES[1][3] > R.CONV_DW_CASES[1][1]
    assert [m > 64 for m, _, _, _, _ in R.CONV_DW_CASES] == [False, True, True, True], "more than one 64-row block"
    assert R.seg_lens(70) == [3, 1, 50, 16] and sum(R.seg_lens(333)) == 333 and R.seg_lens(333)[:5] == [3, 1, 50, 16, 3]
    b, t, c, s, m, ldh, planes, _ = R.CONCAT_CASES[1]
    assert planes and (c + s) % 32 == 0 and m < b * t and ldh > c
    assert [R.ln_maxper(c) for _, c in R.LN_FWD_CASES] == [1, 1, 4, 8, 16]
    assert [R.ln_maxper(c) for _, c, _, _ in R.LN_BWD_CASES] == [4, 8, 16, 1], "65, 257, 513: the first channel count of each wider arm"
    assert R.ln_waves(1029) == (1024, 2) and R.ln_waves(9) == (9, 1) and R.ln_waves(97) == (97, 1), "only M = 1029 gives a wave a second row"
    d = R.ln_inputs(9, 65)
    assert d["pad"][0] == 0 and d["pad"][-1] == 1 and not d["keep"][1].any() and d["keep"][0].any()
