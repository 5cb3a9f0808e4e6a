"""-m gpu: the element-wise and reduction kernels of the training step against their float64 statements (tests/train_pointwise_ref.py), one kernel
call per case: bn_stats_kernel, bn_act_fwd_kernel / bn_act_fwd4_kernel, bn_bwd_kernel / bn_bwd4_kernel, act_fwd_kernel / act_fwd4_kernel,
act_bwd_kernel, colsum_kernel (modes 0..3, out_x, both rows-per-block), conv1d_in1_dw_kernel, unpack_conv_grad_kernel, concat_spk_kernel,
layernorm_kernel and layernorm_bwd_kernel with keep, scalar head and pad mask.

Every case compares each output with the reference within its PER-ELEMENT bound (an element that is a copy or a masked zero must match exactly) and
prints one RATIO line: the worst error / bound per output (HISTORY.md records them per kernel).  Buffers the TEST hands in to be written or accumulated
(running statistics, acc, out, out_x, dw, db, dgamma, dbeta, dlin_w, dlin_b, a workspace) are views between two guard lines of 256 elements of an
all-ones bit pattern, asserted afterwards; outputs the wrappers allocate themselves have none.  Where a four-wide kernel has a scalar twin the case
runs again from operand views one float into their buffers (4-byte, not 16-byte aligned: the scalar kernel) and the two results must be equal bit
for bit.  Inputs go through fcl_taco2_amd.ops, except where the entry point is asked for something ops does not pass on: a NULL y_act, a dirty
workspace, and row strides wider than the row (ops hands over contiguous tensors only).  The inputs and the bounds are checked without a GPU in
tests/test_train_pointwise_ref_cpu.py."""
import numpy as np
import pytest
import torch

import train_pointwise_ref as R
from helpers import max_abs, split_planes_np

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256  # elements of guard in front of and behind every buffer the test hands in to be written


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib, ops as _ops

    _lib.load()
    return _ops


def dev(a):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return t.to(DEV).contiguous()


def off1(a):
    """device copy of `a` as a view R.TWIN_OFFSET floats into a 16-byte aligned buffer: 4-byte aligned, not 16-byte aligned"""
    buf = torch.empty(a.size + 4, device=DEV, dtype=torch.float32)
    v = buf[R.TWIN_OFFSET: R.TWIN_OFFSET + a.size].view(*a.shape)
    v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert buf.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 4 * R.TWIN_OFFSET and v.is_contiguous()
    return v


class Guarded(object):
    """device buffers holding given contents between two guard lines of GUARD elements of all-ones bits"""

    def __init__(self):
        self.bufs = []

    def new(self, name, a):
        a = np.ascontiguousarray(a)
        gb = GUARD * a.itemsize
        full = torch.full((2 * gb + a.nbytes,), 0xFF, device=DEV, dtype=torch.uint8)
        view = full[gb: gb + a.nbytes].view(torch.from_numpy(a).dtype).view(*a.shape)
        view.copy_(torch.from_numpy(a))
        assert view.data_ptr() % 128 == 0
        self.bufs.append((name, full, gb))
        return view

    def check(self):
        for name, full, gb in self.bufs:
            assert bool((full[:gb] == 0xFF).all()) and bool((full[-gb:] == 0xFF).all()), "%s: a guard line was overwritten" % name


def sync():
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:  # a device fault: nothing more may start on this GPU
        pytest.exit("the device reported %s" % e, returncode=3)


def compare(what, got, want, bound):
    """|got - want| <= bound at every element (equality where the bound is 0); returns the worst ratio"""
    got = (got.detach().cpu().numpy() if hasattr(got, "detach") else np.asarray(got)).astype(np.float64)
    want, bound = np.asarray(want, np.float64), np.broadcast_to(np.asarray(bound, np.float64), np.shape(want))
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), "%s: non-finite values" % what
    err, exact = np.abs(got - want), bound == 0
    assert not np.any(exact & (err != 0)), "%s: %d elements that must be exact differ (worst %.3g)" % (what, int(np.sum(exact & (err != 0))), err[exact].max())
    rat = np.where(exact, 0.0, err / np.where(exact, 1.0, bound))
    ratio = float(rat.max()) if got.size else 0.0
    assert ratio <= 1.0, "%s: error / bound %.3f at %s (error %.3g)" % (what, ratio, np.unravel_index(np.argmax(rat), rat.shape), err.max())
    return ratio


def report(kernel, case, ratios):
    print("RATIO %s %s %s" % (kernel, case, " ".join("%s %.3f" % kv for kv in sorted(ratios.items()))))


def same_bits(what, a, b):
    assert a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), "%s: not equal bit for bit (max abs %.3g)" % (what, max_abs(a, b))


def planes_np(p, rows, cols):
    return p.cpu().numpy().view(np.uint16).reshape(rows, (cols + 31) // 32, 2, 32)


# ---- bn_stats ----------------------------------------------------------------------------------------------------------------------------------------
def run_bn_stats(ops, d, g):
    rm = None if d["running_mean"] is None else g.new("running_mean", d["running_mean"])
    rv = None if d["running_var"] is None else g.new("running_var", d["running_var"])
    mean, invstd = ops.bn_stats(dev(d["z"]), R.BN_EPS, d["momentum"], rm, rv)
    sync()
    return dict(mean=mean, invstd=invstd, running_mean=rm, running_var=rv)


def check_bn_stats(d, got):
    ref = R.ref_bn_stats(d["z"], R.BN_EPS, d["momentum"], d["running_mean"], d["running_var"])
    bound = R.bound_bn_stats(d["z"], ref, d["momentum"], d["running_mean"])
    return {k: compare("bn_stats " + k, got[k], ref[k], bound[k]) for k in bound}


@pytest.mark.parametrize("cid", sorted(R.BN_STATS_CASES))
def test_bn_stats(ops, cid):
    d, g = R.bn_stats_inputs(cid), Guarded()
    got = run_bn_stats(ops, d, g)
    g.check()
    ratios = check_bn_stats(d, got)
    eps = np.float64(np.float32(R.BN_EPS))
    assert float(got["invstd"][d["const_col"]]) == np.float32(1.0 / np.sqrt(eps)), "the constant column: var = 0, invstd = 1 / sqrt(eps)"
    report("bn_stats_kernel", cid, ratios)


def test_bn_stats_workspace_is_reset_when_c_changes(ops):
    """C = 130, C = 7, C = 130 on one stream and one workspace: the ticket words sit behind the 2 C sums, so they move with C; every call must leave
    sums and tickets zero, or the next call with another C starts from what the last one left.  The third result equals the first bit for bit."""
    runs = []
    for cid in ("m65_c130", "m257_c7", "m65_c130"):
        d, g = R.bn_stats_inputs(cid), Guarded()
        got = run_bn_stats(ops, d, g)
        g.check()
        runs.append((got, check_bn_stats(d, got)))  # (every result stays alive: no call is handed the memory of an earlier result)
    for k in ("mean", "invstd", "running_mean", "running_var"):
        same_bits("bn_stats %s, third call against the first" % k, runs[2][0][k], runs[0][0][k])
    report("bn_stats_kernel", "reset-130-7-130", runs[2][1])


def test_bn_stats_clears_a_dirty_workspace(ops):
    """fcl_bn_stats_fwd takes any workspace: it clears sums and tickets itself, gives the values of the zero-workspace entry point and leaves zeros"""
    from fcl_taco2_amd import _lib

    d, g, g2 = R.bn_stats_inputs("m65_c130"), Guarded(), Guarded()
    want = run_bn_stats(ops, d, g)
    c = d["c"]
    need = 2 * c + (c + 63) // 64
    ws = g2.new("workspace", np.random.RandomState(0).standard_normal(need) * 1e30)
    mean, invstd = g2.new("mean", np.zeros(c, np.float32)), g2.new("invstd", np.zeros(c, np.float32))
    rm, rv = g2.new("running_mean", d["running_mean"]), g2.new("running_var", d["running_var"])
    z = dev(d["z"])
    _lib.check(_lib.load().fcl_bn_stats_fwd(z.data_ptr(), d["m"], c, R.BN_EPS, d["momentum"], mean.data_ptr(), invstd.data_ptr(), rm.data_ptr(), rv.data_ptr(),
                                            ws.data_ptr(), ops._stream()))
    sync()
    g.check()
    g2.check()
    got = dict(mean=mean, invstd=invstd, running_mean=rm, running_var=rv)
    for k, v in got.items():
        same_bits("bn_stats %s from a dirty workspace" % k, v, want[k])
    assert bool((ws.view(torch.int64) == 0).all()), "the workspace is not left zero"
    report("bn_stats_kernel", "dirty-workspace", check_bn_stats(d, got))


# ---- bn_act ------------------------------------------------------------------------------------------------------------------------------------------
_bn = {}


def bn_case(m, c):
    if (m, c) not in _bn:
        d = R.bn_inputs(m, c)
        _bn[(m, c)] = (d, {k: dev(d[k]) for k in ("z", "mean", "invstd", "gamma", "beta", "dy", "dbeta", "dgamma", "keep")})
    return _bn[(m, c)]


BN_ACT_PARAMS = [(m, c, act, keep) for m, c in R.BN_SHAPES for act in R.BN_ACTS for keep in (False, True)]


@pytest.mark.parametrize("m,c,act,keep", BN_ACT_PARAMS, ids=["m%d_c%d-act%d%s" % (m, c, a, "-keep" if k else "") for m, c, a, k in BN_ACT_PARAMS])
def test_bn_act(ops, m, c, act, keep):
    d, t = bn_case(m, c)
    planes, four = c % 32 == 0, c % 4 == 0
    kn, kt, ks = (d["keep"], t["keep"], R.KEEP_SCALE) if keep else (None, None, 1.0)
    assert all(t[k].data_ptr() % 16 == 0 for k in ("z", "mean", "invstd", "gamma", "beta", "keep"))
    res = ops.bn_act(t["z"], t["mean"], t["invstd"], t["gamma"], t["beta"], act, kt, ks, want_planes=planes)
    sync()
    ref = R.ref_bn_act(d["z"], d["mean"], d["invstd"], d["gamma"], d["beta"], act, kn, ks)
    bound = R.bound_bn_act(ref, d["gamma"], d["beta"], act, kn, ks)
    ratios = dict(y_act=compare("y_act", res[0], ref["y_act"], bound["y_act"]), y_drop=compare("y_drop", res[1], ref["y_drop"], bound["y_drop"]))
    if keep:
        ya, yd = res[0].cpu().numpy(), res[1].cpu().numpy()
        assert np.all(yd[kn == 0] == 0) and np.array_equal(yd[kn != 0], np.float32(2) * ya[kn != 0]), "y_drop is not exactly 0 / 2 y_act"
    if planes:
        assert np.array_equal(planes_np(res[2], m, c), split_planes_np(res[1].cpu().numpy())), "the planes are not the split of y_drop"
    if four:  # the scalar twin: the same operands from views that miss 16-byte alignment
        tw = ops.bn_act(off1(d["z"]), off1(d["mean"]), off1(d["invstd"]), off1(d["gamma"]), off1(d["beta"]), act, kt, ks, want_planes=planes)
        sync()
        for name, a, b in zip(("y_act", "y_drop"), tw, res):
            same_bits("bn_act %s, scalar kernel against four-wide" % name, a, b)
        if planes:
            assert torch.equal(tw[2], res[2]), "bn_act planes, scalar kernel against four-wide"
    report("bn_act_fwd4_kernel+twin" if four else "bn_act_fwd_kernel", "m%d_c%d act%d%s" % (m, c, act, " keep" if keep else ""), ratios)


def test_bn_act_without_y_act(ops):
    """y_act = NULL (the frozen teacher's forward keeps nothing for a backward): y_drop and the planes alone, the same values"""
    from fcl_taco2_amd import _lib

    m, c = 33, 96
    d, t = bn_case(m, c)
    y_act, y_drop, yp = ops.bn_act(t["z"], t["mean"], t["invstd"], t["gamma"], t["beta"], R.ACT_RELU, t["keep"], R.KEEP_SCALE, want_planes=True)
    g = Guarded()
    out = g.new("y_drop", np.zeros((m, c), np.float32))
    outp = g.new("planes", np.zeros((m, c // 32 * 64), np.int16))
    p = lambda k: t[k].data_ptr()  # noqa: E731
    _lib.check(_lib.load().fcl_bn_act_fwd(p("z"), p("mean"), p("invstd"), p("gamma"), p("beta"), p("keep"), R.KEEP_SCALE, None, out.data_ptr(), outp.data_ptr(),
                                          m, c, R.ACT_RELU, ops._stream()))
    sync()
    g.check()
    same_bits("y_drop without y_act", out, y_drop)
    assert torch.equal(outp, yp)
    ref = R.ref_bn_act(d["z"], d["mean"], d["invstd"], d["gamma"], d["beta"], R.ACT_RELU, d["keep"], R.KEEP_SCALE)
    report("bn_act_fwd4_kernel", "m33_c96 y_act=NULL",
           dict(y_drop=compare("y_drop", out, ref["y_drop"], R.bound_bn_act(ref, d["gamma"], d["beta"], R.ACT_RELU, d["keep"], R.KEEP_SCALE)["y_drop"])))


# ---- bn_bwd ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("acc", [False, True], ids=["", "acc"])
@pytest.mark.parametrize("m,c", R.BN_SHAPES)
def test_bn_bwd(ops, m, c, acc):
    d, t = bn_case(m, c)
    planes, four = c % 32 == 0, c % 4 == 0
    g = Guarded()
    accs = (g.new("acc_dbeta", d["acc_dbeta"]), g.new("acc_dgamma", d["acc_dgamma"])) if acc else None
    args = ("dy", "z", "mean", "invstd", "gamma", "dbeta", "dgamma")
    assert all(t[k].data_ptr() % 16 == 0 for k in args)
    res = ops.bn_bwd(*(t[k] for k in args), want_planes=planes, acc=accs)
    sync()
    g.check()
    dz, dzp = res if planes else (res, None)
    ref = R.ref_bn_bwd(*(d[k] for k in args), acc=(d["acc_dbeta"], d["acc_dgamma"]) if acc else None)
    ratios = dict(dz=compare("dz", dz, ref["dz"], R.bound_bn_bwd(ref, d["dy"], d["invstd"], d["gamma"], d["dbeta"], d["dgamma"])))
    if acc:
        compare("acc_dbeta", accs[0], ref["acc_dbeta"], 0.0)
        compare("acc_dgamma", accs[1], ref["acc_dgamma"], 0.0)
    if planes:
        assert np.array_equal(planes_np(dzp, m, c), split_planes_np(dz.cpu().numpy())), "the planes are not the split of dz"
    if four:
        tw = ops.bn_bwd(*(off1(d[k]) for k in args), want_planes=planes)
        sync()
        same_bits("bn_bwd dz, scalar kernel against four-wide", tw[0] if planes else tw, dz)
        if planes:
            assert torch.equal(tw[1], dzp), "bn_bwd planes, scalar kernel against four-wide"
    report("bn_bwd4_kernel+twin" if four else "bn_bwd_kernel", "m%d_c%d%s" % (m, c, " acc" if acc else ""), ratios)


# ---- act_fwd / act_bwd -----------------------------------------------------------------------------------------------------------------------------------
ACT_PARAMS = [(r, c, act, keep) for r, c in R.ACT_SHAPES for act in R.ACTS for keep in (False, True)]


@pytest.mark.parametrize("r,c,act,keep", ACT_PARAMS, ids=["%dx%d-act%d%s" % (r, c, a, "-keep" if k else "") for r, c, a, k in ACT_PARAMS])
def test_act_fwd_and_bwd(ops, r, c, act, keep):
    d = R.act_inputs(r, c)
    planes = c % 32 == 0
    kn, ks = (d["keep"], R.KEEP_SCALE) if keep else (None, 1.0)
    y = ops.act_fwd(dev(d["x"]), act, dev(kn), ks, want_planes=planes)
    dz = ops.act_bwd(dev(d["dy"]), dev(d["y"][act]), act, dev(kn), ks, want_planes=planes)
    sync()
    (y, yp), (dz, dzp) = (y, dz) if planes else ((y, None), (dz, None))
    ref = R.ref_act_fwd(d["x"], act, kn, ks)
    refb = R.ref_act_bwd(d["dy"], d["y"][act], act, kn, ks)
    ratios = dict(y=compare("act_fwd", y, ref, R.bound_act_fwd(ref, act, kn, ks)), dz=compare("act_bwd", dz, refb, R.bound_act_bwd(refb)))
    if keep:
        assert np.all(y.cpu().numpy()[kn == 0] == 0) and np.all(dz.cpu().numpy()[kn == 0] == 0), "masked elements are not exactly zero"
    if planes:
        assert np.array_equal(planes_np(yp, r, c), split_planes_np(y.cpu().numpy())) and np.array_equal(planes_np(dzp, r, c), split_planes_np(dz.cpu().numpy()))
    report("act_fwd4_kernel,act_bwd_kernel" if (r * c) % 4 == 0 else "act_fwd_kernel,act_bwd_kernel", "%dx%d act%d%s" % (r, c, act, " keep" if keep else ""), ratios)


# ---- colsum ------------------------------------------------------------------------------------------------------------------------------------------
_cs = {}
COLSUM_PARAMS = [(m, c, mode, ox) for m, c in R.COLSUM_SHAPES for mode in range(4) for ox in (False, True)]


@pytest.mark.parametrize("m,c,mode,with_x", COLSUM_PARAMS, ids=["m%d_c%d-mode%d%s" % (m, c, md, "-out_x" if ox else "") for m, c, md, ox in COLSUM_PARAMS])
def test_colsum(ops, m, c, mode, with_x):
    if (m, c) not in _cs:
        _cs.clear()
        d = R.colsum_inputs(m, c)
        _cs[(m, c)] = (d, {k: dev(d[k]) for k in ("x", "y", "g", "b")})
    d, t = _cs[(m, c)]
    g = Guarded()
    out = g.new("out", d["out"])
    out_x = g.new("out_x", d["out_x"]) if with_x else None
    ops.colsum(t["x"], out, y=t["y"] if mode >= 1 else None, gamma=t["g"] if mode >= 2 else None, beta=t["b"] if mode >= 2 else None, mode=mode, out_x=out_x)
    sync()
    g.check()
    terms = R.colsum_terms(d["x"], d["y"], d["g"], d["b"], mode)
    ratios = dict(out=compare("colsum", out, R.ref_colsum(terms, d["out"]), R.bound_colsum(terms, d["out"])))
    if with_x:
        tx = R.colsum_terms(d["x"])
        ratios["out_x"] = compare("colsum out_x", out_x, R.ref_colsum(tx, d["out_x"]), R.bound_colsum(tx, d["out_x"]))
    report("colsum_kernel/rpb%d" % R.rows_per_block(m), "m%d_c%d mode%d" % (m, c, mode), ratios)


# ---- conv1d_in1_dw -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,c,k,ldy,full", R.CONV_DW_CASES, ids=["m%d_c%d_k%d_ld%d" % cs[:4] for cs in R.CONV_DW_CASES])
def test_conv1d_in1_dw(ops, m, c, k, ldy, full):
    from fcl_taco2_amd import _lib

    d, g = R.conv_dw_inputs(m, c, k, ldy, full), Guarded()
    dy_buf, x = dev(d["dy_buf"]), dev(d["x"])
    lo, hi = dev(d["seg_lo"]), dev(d["seg_hi"])
    dw = g.new("dw", d["dw"])
    db = g.new("db", d["db"]) if full else None
    if ldy == c:
        ops.conv1d_in1_dw(dy_buf, x, dw, db, seg_lo=lo, seg_hi=hi)
    else:  # a row stride wider than the row: ops passes contiguous tensors only
        p = lambda v: None if v is None else v.data_ptr()  # noqa: E731
        _lib.check(_lib.load().fcl_conv1d_in1_dw(p(dy_buf), ldy, p(x), p(lo), p(hi), p(dw), p(db), m, c, k, ops._stream()))
    sync()
    g.check()
    ref = R.ref_conv1d_in1_dw(d["dy_buf"][:, :c], d["x"], k, d["dw"][:, 0, :], d["db"], d["seg_lo"], d["seg_hi"])
    ratios = dict(dw=compare("dw", dw[:, 0, :], ref["dw"], ref["bound_dw"]))
    if full:
        ratios["db"] = compare("db", db, ref["db"], ref["bound_db"])
    report("conv1d_in1_dw_kernel", "m%d_c%d_k%d_ld%d" % (m, c, k, ldy), ratios)


# ---- unpack_conv1d_grad ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scaled", [False, True], ids=["", "scale"])
@pytest.mark.parametrize("cout,cin,k", R.UNPACK_SHAPES)
def test_unpack_conv1d_grad(ops, cout, cin, k, scaled):
    d, g = R.unpack_inputs(cout, cin, k), Guarded()
    dw = g.new("dw", d["dw"])
    ops.unpack_conv1d_grad(dev(d["dwp"]), dw, scale=dev(d["scale"]) if scaled else None)
    sync()
    g.check()
    ref, bound = R.ref_unpack(d["dwp"], d["dw"], d["scale"] if scaled else None)
    report("unpack_conv_grad_kernel", "%dx%dx%d%s" % (cout, cin, k, " scale" if scaled else ""), dict(dw=compare("dw", dw, ref, bound)))


# ---- concat_spk --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CONCAT_CASES, ids=lambda cs: "c%d_s%d" % (cs[2], cs[3]))
def test_concat_spk(ops, case):
    from fcl_taco2_amd import _lib

    b, t, c, s, m, ldh, planes, kinds = case
    d = R.concat_inputs(*case)
    hs_buf, spk = dev(d["hs_buf"]), dev(d["spk"])
    if ldh == c:
        out, outp = ops.concat_spk(hs_buf, spk, t, want_planes=planes)
    else:  # hs is a column view of a wider buffer: ops passes contiguous tensors only
        out = torch.empty(m, c + s, device=DEV)
        outp = ops.planes_empty(m, c + s, DEV) if planes else None
        _lib.check(_lib.load().fcl_concat_spk_fwd(hs_buf.data_ptr(), ldh, spk.data_ptr(), out.data_ptr(), outp.data_ptr() if planes else None, m, c, s, t,
                                                  ops._stream()))
    sync()
    ref, bound = R.ref_concat_spk(d["hs_buf"][:, :c], d["spk"], t)
    ratios = dict(out=compare("concat_spk", out, ref, bound))
    for i, kind in enumerate(kinds):
        if kind == "zero" and i * t < m:
            assert bool((out[i * t: min(m, (i + 1) * t), c:] == 0).all()), "an all-zero speaker vector must give exact zeros"
    if planes:
        assert np.array_equal(planes_np(outp, m, c + s), split_planes_np(out.cpu().numpy())), "the planes are not the split of out"
    report("concat_spk_kernel", "c%d_s%d_m%d" % (c, s, m), ratios)


# ---- layernorm forward / backward ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,c", R.LN_FWD_CASES)
def test_layernorm_fwd(ops, m, c):
    d = R.ln_inputs(m, c)
    planes = c in (20, 64)
    res = ops.layernorm(dev(d["x"]), dev(d["gamma"]), dev(d["beta"]), R.LN_EPS, True, dev(d["lin_w"]), dev(d["lin_b"]), dev(d["pad"]), dev(d["keep"]), R.KEEP_SCALE,
                        want_planes=planes)
    sync()
    ref = R.ref_layernorm(d["x"], d["gamma"], d["beta"], R.LN_EPS, d["keep"], R.KEEP_SCALE, d["lin_w"], d["lin_b"], d["pad"])
    ratios = dict(y=compare("y", res[0], ref["y"], ref["tol_y"]), scalar=compare("scalar", res[1], ref["scalar"], ref["tol_s"]))
    if planes:  # C = 20: the last 32-column line is zero-padded (split_planes_np pads with zeros)
        assert np.array_equal(planes_np(res[2], m, c), split_planes_np(res[0].cpu().numpy())), "the planes are not the split of the zero-padded y"
    report("layernorm_kernel<%d>" % R.ln_maxper(c), "m%d_c%d keep head pad" % (m, c), ratios)


@pytest.mark.parametrize("m,c,with_dy,with_ds", R.LN_BWD_CASES, ids=["m%d_c%d%s%s" % (m, c, "" if a else "-head_only", "" if b else "-no_head") for m, c, a, b in R.LN_BWD_CASES])
def test_layernorm_bwd(ops, m, c, with_dy, with_ds):
    d, g = R.ln_inputs(m, c), Guarded()
    names = ("dgamma", "dbeta") + (("dlin_w", "dlin_b") if with_ds else ())
    acc = {k: g.new(k, d["before"][k]) for k in names}
    dx = ops.layernorm_bwd(dev(d["x"]), dev(d["gamma"]), dev(d["beta"]), R.LN_EPS, acc["dgamma"], acc["dbeta"], dy=dev(d["dy"]) if with_dy else None,
                           lin_w=dev(d["lin_w"]) if with_ds else None, ds=dev(d["ds"]) if with_ds else None, pad_mask=dev(d["pad"]), dlin_w=acc.get("dlin_w"),
                           dlin_b=acc.get("dlin_b"), keep=dev(d["keep"]), keep_scale=R.KEEP_SCALE)
    sync()
    g.check()
    ref = R.ref_layernorm_bwd(d["x"], d["gamma"], d["beta"], R.LN_EPS, dy=d["dy"] if with_dy else None, lin_w=d["lin_w"] if with_ds else None,
                              ds=d["ds"] if with_ds else None, pad=d["pad"], keep=d["keep"], keep_scale=R.KEEP_SCALE, before=d["before"])
    ratios = dict(dx=compare("dx", dx, ref["dx"], ref["bound_dx"]))
    for k in names:
        ratios[k] = compare(k, acc[k], ref[k], ref["bound_" + k])
    report("layernorm_bwd_kernel<%d>" % R.ln_maxper(c), "m%d_c%d rows/wave %d" % (m, c, R.ln_waves(m)[1]), ratios)
