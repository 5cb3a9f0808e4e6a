"""The float64 statement of the HiFi-GAN scale discriminators (tests/hfgs_ref.py) against torch, its bounds against a float32 evaluation and
against mutants, and everything of fcl_taco2_amd/hifigan_scale_discriminator.py that needs no GPU: the refusals, the names, the spectral-norm holder, the
plan's geometry, the pooled lengths, the C entries' argument checks.

Shares of unsure cells, measured on exactly the GPU test's arrays at gain 1/4 (the cases print them): chain A at most 0.54 % (its last map), chain B 0.28 %;
the multi-scale case (MSD_CFG, three scales, mask and L1 kinks together) 0.50 %."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import hfgd_ref as D
import hfgs_ref as R
from conftest import ROOT


@pytest.fixture(scope="module")
def P():
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import hifigan_scale_discriminator

    return hifigan_scale_discriminator


@functools.lru_cache(maxsize=None)
def case(name):
    return R.chain_case(name)


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def share(diff, bound):
    return float(np.max(np.abs(diff) / np.maximum(bound, 1e-300)))


@pytest.mark.parametrize("name", ["A", "B"])
def test_numpy_statement_agrees_with_the_torch_statement(name):
    c = case(name)
    ts = R.torch_statement(c["cfg"], c["ws"], c["xs"], c["ds"], c["ex"])
    for r, th in zip(c["fw"], ts["h"]):
        assert [a.shape for a in r["h"]] == [b.shape for b in th]
        assert max(rel(a, b) for a, b in zip(r["h"], th)) <= 1e-12
    bw = c["bw"]
    assert max(rel(a, b) for a, b in zip(bw["gx"], ts["gx"])) <= 1e-12
    assert max(rel(a, b) for a, b in zip(bw["dw"], ts["dw"])) <= 1e-12 and max(rel(a, b) for a, b in zip(bw["db"], ts["db"])) <= 1e-12
    plain = R.backward(c["cfg"], c["ws"], c["fw"], c["ds"])  # without the direct feature-map gradients
    tp = R.torch_statement(c["cfg"], c["ws"], c["xs"], c["ds"])
    assert max(rel(a, b) for a, b in zip(plain["gx"], tp["gx"])) <= 1e-12 and max(rel(a, b) for a, b in zip(plain["dw"], tp["dw"])) <= 1e-12
    assert rel(plain["gx"][2], bw["gx"][2]) > 1e-3


def test_pooling_and_its_adjoint_agree_with_torch_and_the_pooled_lengths(P):
    import torch.nn.functional as F

    for T, want in ((1, 1), (2, 2), (3, 2), (4, 3), (5, 3), (130, 66), (401, 201)):
        x = R.signals([T], T)[0]
        xt = torch.tensor(x, requires_grad=True)
        y = F.avg_pool1d(xt[None, None], 4, 2, 2)[0, 0]
        assert len(y) == want == R.pooled_length(T) == P.pooled_length(T) == len(R.pool(x))
        assert np.allclose(R.pool(x), y.detach().numpy(), rtol=1e-14, atol=1e-17)
        g = R.normal((want,), T)
        (y * torch.tensor(g)).sum().backward()
        assert np.allclose(R.pool_adjoint(g, T), xt.grad.numpy(), rtol=1e-14, atol=1e-17)
    # a chain of two poolings in front of the stack, against avg_pool1d twice, gradient to the unpooled waveform included
    c = case("B")
    xs = c["xs"][:3]
    chains = [R.pool_chain(x, 2) for x in xs]
    fw = R.forward(c["cfg"], c["ws"], [ch[2][0] for ch in chains])
    ds, ex = R.given_gradients(fw, 5)
    bw = R.backward(c["cfg"], c["ws"], fw, ds, extras=ex)
    ts = R.torch_statement(c["cfg"], c["ws"], xs, ds, ex, pooled=2)
    assert max(rel(ch[2][0], v) for ch, v in zip(chains, ts["x"])) <= 1e-13
    for g, ch, want in zip(bw["gx"], chains, ts["gx"]):
        assert rel(R.pool_adjoint(R.pool_adjoint(g, len(ch[1][0])), len(ch[0][0])), want) <= 1e-12


def holder_and_torch(P, shape, groups, seed):
    """the package's holder and torch.nn.utils.spectral_norm on a Conv1d from the same weight_orig, u, v (float64)"""
    torch.manual_seed(seed)
    co, cig, k = shape
    mine = P._SpectralConv(shape, True).double()
    conv = torch.nn.utils.spectral_norm(torch.nn.Conv1d(cig * groups, co, k, groups=groups).double())
    with torch.no_grad():
        conv.weight_orig.copy_(mine.weight_orig), conv.weight_u.copy_(mine.weight_u), conv.weight_v.copy_(mine.weight_v), conv.bias.copy_(mine.bias)
    return mine, conv


@pytest.mark.parametrize("shape,groups", [((32, 8, 11), 4), ((16, 1, 5), 1), ((1, 32, 3), 1)])
def test_spectral_norm_holder_agrees_with_torch(P, shape, groups):
    mine, conv = holder_and_torch(P, shape, groups, 3)
    assert sorted(mine.state_dict()) == sorted(conv.state_dict()) == ["bias", "weight_orig", "weight_u", "weight_v"]
    assert [tuple(v.shape) for _, v in sorted(mine.state_dict().items())] == [tuple(v.shape) for _, v in sorted(conv.state_dict().items())]
    W0, u0, v0 = (a.detach().numpy().copy() for a in (mine.weight_orig, mine.weight_u, mine.weight_v))
    x = torch.randn(1, shape[1] * groups, 20, dtype=torch.float64)
    # one training forward: the folded weight, the buffers after the iteration, the gradient of a scalar with respect to weight_orig
    w = mine.folded()
    conv(x)
    assert torch.allclose(w, conv.weight, rtol=1e-13, atol=0)
    assert torch.allclose(mine.weight_u, conv.weight_u, rtol=1e-13, atol=1e-16) and torch.allclose(mine.weight_v, conv.weight_v, rtol=1e-13, atol=1e-16)
    assert not np.allclose(mine.weight_v.numpy(), v0)
    probe = torch.randn_like(w)
    (w * probe).sum().backward()
    (conv.weight * probe).sum().backward()
    assert torch.allclose(mine.weight_orig.grad, conv.weight_orig.grad, rtol=1e-12, atol=1e-15)
    # the numpy statement: the iteration, sigma, the fold, the gradient with u, v held constant; the mutant's sigma is the one before the iteration
    wf, u1, v1 = R.spectral_fold(W0, u0, v0, training=True)
    assert rel(wf, w.detach().numpy()) <= 1e-13 and rel(u1, mine.weight_u.numpy()) <= 1e-13 and rel(v1, mine.weight_v.numpy()) <= 1e-13
    assert rel(R.spectral_gradient(W0, u1, v1, probe.numpy()), mine.weight_orig.grad.numpy()) <= 1e-12
    assert rel(R.spectral_fold(W0, u0, v0, training=True, mutant="sigma_before_iteration")[0], wf) > 1e-3
    # eval: no iteration, the buffers stay
    mine.eval(), conv.eval()
    keep = (mine.weight_u.clone(), mine.weight_v.clone())
    w2 = mine.folded()
    conv(x)
    assert torch.allclose(w2, conv.weight, rtol=1e-13, atol=0) and torch.equal(mine.weight_u, keep[0]) and torch.equal(mine.weight_v, keep[1])
    assert rel(R.spectral_fold(W0, u1, v1)[0], w2.detach().numpy()) <= 1e-13


def to32(a):
    return None if a is None else np.asarray(a, dtype=np.float32)


@pytest.mark.parametrize("name", ["A", "B"])
def test_a_float32_evaluation_stays_inside_every_bound_and_the_cap_holds_per_array(name):
    """on exactly the GPU test's arrays: the unsure share of every map at most CAP, no running gradient bound above its peak, and the statement itself
    evaluated in float32 (masks from its own float32 activations, as the device's) inside the running bounds"""
    c = case(name)
    shares = R.unsure_shares(c["fw"])
    bw = c["bw"]
    print("chain %s at gain %g: unsure share per map %s, gradient bound / peak %s, dW bound / peak %s" % (name, R.GAIN, np.round(shares, 5), np.round(
        [b / k for b, k in zip(bw["g_bound"], bw["g_peak"])], 3), np.round([e.max() / np.abs(d).max() for e, d in zip(bw["dw_e"], bw["dw"])], 3)))
    assert max(shares) <= R.CAP
    assert all(b <= k for b, k in zip(bw["g_bound"], bw["g_peak"])) and all(e.max() <= np.abs(g).max() for e, g in zip(bw["gx_e"], bw["gx"]))
    ws32 = [(to32(W), to32(b)) for W, b in c["ws"]]
    xs32 = [to32(x) for x in c["xs"]]
    fw32 = R.forward(c["cfg"], ws32, xs32)
    for r, q in zip(c["fw"], fw32):
        assert all(a.dtype == np.float32 for a in q["h"])
        assert max(share(a.astype(np.float64) - b, e) for a, b, e in zip(q["h"], r["h"], r["e"])) <= 1.0
    b32 = R.backward(c["cfg"], ws32, fw32, [to32(d) for d in c["ds"]], extras=[[to32(e) for e in ex] for ex in c["ex"]])
    assert b32["dw"][1].dtype == np.float32
    assert max(share(np.linalg.norm(a - b), np.linalg.norm(e)) for a, b, e in zip(b32["gx"], bw["gx"], bw["gx_e"])) <= 1.0
    for key in ("dw", "db"):
        assert max(share(a.astype(np.float64) - b, e) for a, b, e in zip(b32[key], bw[key], bw[key + "_e"])) <= 1.0, key


def test_the_multi_scale_case_stays_under_the_cap_and_agrees_with_torch():
    """the L1-cell share is measured here first: MSD_CFG is the configuration that gave way until every map of every scale stayed under the cap"""
    import torch.nn.functional as F

    m = R.msd_case()
    ref, cfg = m["ref"], m["cfg"]
    print("multi-scale case: (scale, map, unsure share, mask cells alone) %s" % [(i, l, round(a, 5), round(b, 5)) for i, l, a, b in ref["shares"]])
    assert ref["unsure"] <= R.CAP
    assert max(np.linalg.norm(e) / np.linalg.norm(g) for e, g in zip(ref["gx_e"], ref["gx"])) < 1.0
    assert all(0 < ref[k + "_e"] < abs(ref[k]) for k in ("adv", "fm", "d_real", "d_fake"))
    # the three losses and the whole generator gradient against autograd through conv1d(groups=) and avg_pool1d
    geo = R.geometry(cfg)
    xs = [torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in m["fake"]]

    def outs(waves, ws, pooled):
        maps = [[] for _ in geo]
        for x in waves:
            h = x[None, None, :]
            for _ in range(pooled):
                h = F.avg_pool1d(h, 4, 2, 2)
            for l, (ci, co, k, s, pad, gr) in enumerate(geo):
                h = F.conv1d(h, torch.tensor(ws[l][0]), torch.tensor(ws[l][1]), stride=s, padding=pad, groups=gr)
                h = F.leaky_relu(h, cfg["negative_slope"]) if l < len(geo) - 1 else h
                maps[l].append(h[0].T.reshape(-1))
        return [torch.cat(v) for v in maps]

    reals = [torch.tensor(x, dtype=torch.float64) for x in m["real"]]
    o_r, o_f = [outs(reals, ws, i) for i, ws in enumerate(m["wss"])], [outs(xs, ws, i) for i, ws in enumerate(m["wss"])]
    adv, fm, d_real, d_fake = D.torch_losses(o_r, o_f)
    for got, key in ((adv, "adv"), (fm, "fm"), (d_real, "d_real"), (d_fake, "d_fake")):
        assert abs(got.item() - ref[key]) <= 1e-12 * abs(ref[key])
    (adv + 2.0 * fm).backward()
    assert max(rel(g, x.grad.numpy()) for g, x in zip(ref["gx"], xs)) <= 1e-12


def test_the_combined_reference_averages_over_scales_and_periods():
    m = R.msd_case()
    periods = (2, 3)
    wss_p = [D.weights(D.MPD_CFG, 20 + i) for i in range(len(periods))]
    both = R.combined_reference(m["cfg"], m["wss"], D.MPD_CFG, wss_p, m["real"], m["fake"], periods)
    per = D.mpd_reference(D.MPD_CFG, wss_p, m["real"], m["fake"], periods)
    for key in ("adv", "fm", "d_real", "d_fake"):
        assert both[key] == pytest.approx((3 * m["ref"][key] + 2 * per[key]) / 5, rel=1e-12)
    assert rel(both["gx"][1], (3 * m["ref"]["gx"][1] + 2 * per["gx"][1]) / 5) <= 1e-12


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_violates_a_bound(mutant):
    c = case("A")
    cfg, ws, xs, fw, bw = c["cfg"], c["ws"], c["xs"], c["fw"], c["bw"]
    if mutant == "sigma_before_iteration":
        W = ws[1][0]
        u, v = R.spectral_state(W, 1, iterations=1)
        want, e = R.spectral_fold(W, u, v, training=True)[0], R.spectral_w_ulps(W, u, v) * R.U
        worst = share(R.spectral_fold(W, u, v, training=True, mutant=mutant)[0] - want, e * np.abs(want))
    elif mutant in ("pooled_length_floor", "stride_plus_one"):  # the shapes differ already
        if mutant == "pooled_length_floor":
            assert all(len(R.pool(x, mutant)) != len(R.pool(x)) for x in xs)
        else:
            assert any(a["h"][-1].shape != b["h"][-1].shape for a, b in zip(R.forward(cfg, ws, xs, mutant), fw))
        return
    elif mutant.startswith("pool_"):
        worst = max(share(R.pool(x, mutant) - R.pool(x), R.pool_bound(x, np.zeros_like(x))) for x in xs)
    else:
        worst = 0.0
        if mutant in ("groups_ignored", "membership_modulo", "across_boundary"):
            mf = R.forward(cfg, ws, xs, mutant)
            worst = max(share(a - b, e) for q, r in zip(mf, fw) for a, b, e in zip(q["h"], r["h"], r["e"]))
        if mutant != "across_boundary":
            mb = R.backward(cfg, ws, fw, c["ds"], extras=c["ex"], mutant=mutant)
            worst = max([worst] + [share(np.linalg.norm(a - b), np.linalg.norm(e)) for a, b, e in zip(mb["gx"], bw["gx"], bw["gx_e"])])
    assert worst > 1.0, (mutant, worst)


def test_check_configuration_refuses_each_unsupported_argument_by_name(P):
    assert P.check_configuration() == [(1, 128, 15, 1, 7, 1), (128, 128, 41, 2, 20, 4), (128, 256, 41, 2, 20, 16), (256, 512, 41, 4, 20, 16),
                                       (512, 1024, 41, 4, 20, 16), (1024, 1024, 41, 1, 20, 16), (1024, 1024, 5, 1, 2, 1), (1024, 1, 3, 1, 1, 1)]
    for cfg in (R.CHAIN_A, R.CHAIN_B, R.MSD_CFG):
        assert P.check_configuration(**cfg) == R.geometry(cfg)
    assert P.layer_kinds(R.geometry(R.CHAIN_A)) == ["first", "grouped", "grouped", "dense", "score"]
    bad = dict(in_channels=2, out_channels=2, kernel_sizes=(17, 41, 5, 3), channels=32, downsample_scales=(5,), max_downsample_channels=2048, max_groups=0, bias=None,
               nonlinear_activation="ReLU", negative_slope=1.0, use_weight_norm="yes", use_spectral_norm=True)
    for name, value in bad.items():
        with pytest.raises(ValueError, match=name + "="):
            P.check_configuration(**{name: value})
    for more in (dict(kernel_sizes=(15, 43, 5, 3)), dict(kernel_sizes=(15, 40, 5, 3)), dict(kernel_sizes=(15, 41, 7, 3)), dict(kernel_sizes=(15, 41, 5, 5)),
                 dict(kernel_sizes=(15, 41, 5)), dict(kernel_sizes=(1, 41, 5, 3)), dict(channels=1040), dict(channels=24), dict(downsample_scales=()),
                 dict(downsample_scales=(1,) * 9), dict(downsample_scales=(0,)), dict(negative_slope=-0.1), dict(max_downsample_channels=8),
                 dict(max_groups=64), dict(channels=64, max_groups=16)):  # 64 -> 128 in 16 groups: 8 output channels per group
        with pytest.raises(ValueError, match=list(more)[-1] + "="):
            P.check_configuration(**more)
    assert P.check_configuration(use_weight_norm=False, use_spectral_norm=True)[0] == (1, 128, 15, 1, 7, 1)
    with pytest.raises(ValueError, match="channels=100"):
        P.HiFiGANMultiScaleDiscriminator(discriminator_params=dict(channels=100))
    for kw, name in ((dict(scales=0), "scales"), (dict(scales=5), "scales"), (dict(downsample_pooling="MaxPool1d"), "downsample_pooling"),
                     (dict(downsample_pooling_params={"kernel_size": 4, "stride": 2, "padding": 1}), "downsample_pooling_params"),
                     (dict(follow_official_norm=None), "follow_official_norm")):
        with pytest.raises(ValueError, match=name + "="):
            P.HiFiGANMultiScaleDiscriminator(discriminator_params=dict(R.MSD_CFG), **kw)
    with pytest.raises(ValueError, match="scale_downsample_pooling|downsample_pooling="):
        P.HiFiGANMultiScaleMultiPeriodDiscriminator(scale_downsample_pooling="MaxPool1d")
    from fcl_taco2_amd import _lib

    with pytest.raises(_lib.FclError, match="no CPU fallback"):
        P.HiFiGANMultiScaleDiscriminator(discriminator_params=dict(R.MSD_CFG))(torch.zeros(2, 100))


def test_plan_geometry_and_kept_bytes(P):
    plan = P.ScalePlan.__new__(P.ScalePlan)
    plan.geometry, plan.layers = P.check_configuration(**R.CHAIN_A), 5
    assert plan.heights(1) == [1, 1, 1, 1, 1, 1] and plan.heights(1100) == [1100, 1100, 550, 138, 138, 138] and plan.heights(77) == [77, 77, 39, 10, 10, 10]
    rows = plan.rows(R.LENS)
    per = [R.forward(R.CHAIN_A, R.weights(R.CHAIN_A, 0), [np.zeros(n)])[0] for n in R.LENS]
    assert rows[0] == sum(R.LENS) and rows[1:] == [sum(r["h"][l].shape[1] for r in per) for l in range(5)]
    assert plan.act_shapes(rows) == [(rows[1], 128), (rows[2], 128), (rows[3], 256), (rows[4], 256), (rows[5],)]
    assert plan.kept_bytes(R.LENS) == 4 * (rows[0] + 128 * (rows[1] + rows[2]) + 256 * (rows[3] + rows[4]))
    assert plan.dweight_shapes() == [((5, 1, 128), (128,)), ((11, 32, 128), (128,)), ((11, 8, 256), (256,)), ((3, 256, 256), (256,)), ((3, 256, 1), (1,))]


def test_state_dict_names_shapes_and_round_trips(P):
    names = lambda i, form: ["%slayers.%d.0.%s" % (i, l, n) for l in range(7) for n in form] + ["%slayers.7.%s" % (i, n) for n in form]
    wn, sn, plain = ("weight_g", "weight_v", "bias"), ("weight_orig", "weight_u", "weight_v", "bias"), ("weight", "bias")
    one = P.HiFiGANScaleDiscriminator()
    sd = one.state_dict()
    assert sorted(sd) == sorted(names("", wn))
    shapes = [(128, 1, 15), (128, 32, 41), (256, 8, 41), (512, 16, 41), (1024, 32, 41), (1024, 64, 41), (1024, 1024, 5)]
    assert [tuple(sd["layers.%d.0.weight_v" % l].shape) for l in range(7)] == shapes and sd["layers.7.weight_v"].shape == (1, 1024, 3)
    assert sd["layers.2.0.weight_g"].shape == (256, 1, 1) and sd["layers.2.0.bias"].shape == (256,) and sd["layers.7.bias"].shape == (1,)
    spec = P.HiFiGANScaleDiscriminator(use_weight_norm=False, use_spectral_norm=True).state_dict()
    assert sorted(spec) == sorted(names("", sn)) and spec["layers.2.0.weight_orig"].shape == (256, 8, 41)
    assert spec["layers.2.0.weight_u"].shape == (256,) and spec["layers.2.0.weight_v"].shape == (8 * 41,) and spec["layers.7.weight_v"].shape == (1024 * 3,)
    del one, sd, spec
    small = dict(R.MSD_CFG)
    msd = P.HiFiGANMultiScaleDiscriminator(discriminator_params=small)
    assert sorted(msd.state_dict()) == sorted(n for i in range(3) for n in _small_names("discriminators.%d." % i, wn))
    off = P.HiFiGANMultiScaleDiscriminator(discriminator_params=small, follow_official_norm=True)
    assert sorted(off.state_dict()) == sorted(_small_names("discriminators.0.", sn) + [n for i in (1, 2) for n in _small_names("discriminators.%d." % i, wn)])
    both = P.HiFiGANMultiScaleMultiPeriodDiscriminator(scale_discriminator_params=small, periods=(2, 3), period_discriminator_params=dict(D.SMALL))
    sdb = both.state_dict()
    assert sorted(k for k in sdb if k.startswith("msd.")) == sorted("msd." + k for k in off.state_dict())
    assert sorted(k for k in sdb if k.startswith("mpd.")) == sorted(
        "mpd." + k for k in P.HiFiGANMultiPeriodDiscriminator(periods=(2, 3), discriminator_params=dict(D.SMALL)).state_dict()) and len(sdb) == sum(
        k.startswith(("msd.", "mpd.")) for k in sdb)
    assert both.CHECKPOINT_KEY == msd.CHECKPOINT_KEY == "discriminator"
    # round trips: a whole checkpoint into the same form; a weight-norm dict into a plain module is folded; spectral-norm entries load as they are
    again = P.HiFiGANMultiScaleMultiPeriodDiscriminator(scale_discriminator_params=small, periods=(2, 3), period_discriminator_params=dict(D.SMALL))
    again.load_state_dict({"model": {"generator": {}, "discriminator": sdb}})
    assert all(torch.equal(v, again.state_dict()[k]) for k, v in sdb.items())
    bare = P.HiFiGANMultiScaleDiscriminator(discriminator_params=dict(small, use_weight_norm=False))
    assert sorted(bare.state_dict()) == sorted(n for i in range(3) for n in _small_names("discriminators.%d." % i, plain))
    bare.load_state_dict(msd.state_dict())
    for da, db in zip(msd.discriminators, bare.discriminators):
        for ma, mb in zip(da.conv_list(), db.conv_list()):
            assert torch.equal(ma.folded(), mb.weight)
    msd2 = P.HiFiGANMultiScaleDiscriminator(discriminator_params=small)
    msd2.load_state_dict(bare.state_dict())
    for db, d2 in zip(bare.discriminators, msd2.discriminators):
        for mb, m2 in zip(db.conv_list(), d2.conv_list()):
            assert torch.allclose(m2.folded(), mb.weight, rtol=1e-6, atol=0)
    msd.remove_weight_norm()
    assert sorted(msd.state_dict()) == sorted(bare.state_dict()) and all(torch.equal(msd.state_dict()[k], bare.state_dict()[k]) for k in bare.state_dict())


def _small_names(prefix, form):
    """MSD_CFG has three activated layers and the score layer"""
    return ["%slayers.%d.0.%s" % (prefix, l, n) for l in range(3) for n in form] + ["%slayers.3.%s" % (prefix, n) for n in form]


def test_c_entries_validate_without_a_gpu(tmp_path):
    import __graft_entry__ as ge

    ge.build()
    from fcl_taco2_amd import _lib

    lib = _lib.load()
    entries = (lib.fcl_hsd_layer_fwd, lib.fcl_hsd_layer_dx, lib.fcl_hsd_layer_dw)
    for f in entries:
        assert f(None, None) == -1 and b"null" in lib.fcl_last_error()

    def layer(**kw):
        a = _lib.HsdLayer()
        a.rows_in, a.rows_out, a.cin, a.cout, a.groups, a.ksize, a.stride, a.pad, a.slope = 300, 150, 128, 256, 16, 41, 2, 20, 0.1
        for n in ("src", "in_lo", "in_hi", "x", "w", "bias", "h", "g", "extra", "y", "dw", "db", "workspace"):
            setattr(a, n, 256)
        a.workspace_bytes = 1 << 30
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for f in entries:
        for bad in (dict(cin=120), dict(cout=1040), dict(cin=1, cout=1), dict(cout=1), dict(cin=2), dict(cout=0)):
            assert f(C.byref(layer(**bad)), None) == -2 and b"multiples of 16" in lib.fcl_last_error(), bad
        for bad in (dict(groups=0), dict(groups=3), dict(groups=32), dict(cin=64, groups=16), dict(cin=1, groups=4, ksize=15, pad=7)):
            assert f(C.byref(layer(**bad)), None) == -2 and b"group" in lib.fcl_last_error(), bad
        for bad in (dict(ksize=4, pad=1), dict(ksize=43, pad=21), dict(ksize=1, pad=0), dict(stride=0), dict(stride=5), dict(pad=19),
                    dict(cin=1, groups=1, ksize=17, pad=8)):
            assert f(C.byref(layer(**bad)), None) == -2 and b"kernel size" in lib.fcl_last_error(), bad
        assert f(C.byref(layer(rows_in=0)), None) == -2 and f(C.byref(layer(rows_out=2 ** 31)), None) == -2 and b"rows" in lib.fcl_last_error()
        assert f(C.byref(layer(slope=1.0)), None) == -1 and b"slope" in lib.fcl_last_error()
        for n in ("src", "in_lo", "in_hi"):
            assert f(C.byref(layer(**{n: None})), None) == -1
    fwd, dx, dw = entries
    for n in ("x", "w", "y"):
        assert fwd(C.byref(layer(**{n: None})), None) == -1
        assert fwd(C.byref(layer(**{n: 260})), None) == -3 and b"16-byte" in lib.fcl_last_error()
    for n in ("g", "w", "y", "h"):
        assert dx(C.byref(layer(**{n: None})), None) == -1
    first = dict(cin=1, groups=1, ksize=15, pad=7)
    assert dx(C.byref(layer(extra=None, **first)), None) == -1 and b"first layer" in lib.fcl_last_error()  # h has no meaning there
    assert dx(C.byref(layer(h=None, **first)), None) == -1
    assert dx(C.byref(layer(g=264)), None) == -3 and dx(C.byref(layer(extra=264)), None) == -3
    for n in ("x", "g", "dw", "workspace"):
        assert dw(C.byref(layer(**{n: None})), None) == -1
    need = lib.fcl_hsd_dw_workspace_bytes(150, 128, 256, 16, 41)
    assert need == 1 * (41 * 8 + 1) * 256 * 4 and lib.fcl_hsd_dw_workspace_bytes(1025, 1, 128, 1, 15) == 2 * 16 * 128 * 4
    assert lib.fcl_hsd_dw_workspace_bytes(2049, 1024, 1024, 16, 41) == 3 * (41 * 64 + 1) * 1024 * 4 and lib.fcl_hsd_dw_workspace_bytes(0, 64, 64, 4, 3) == 0
    assert lib.fcl_hsd_dw_workspace_bytes(100, 64, 64, 3, 3) == 0
    assert dw(C.byref(layer(workspace_bytes=need - 4)), None) == -5 and b"workspace" in lib.fcl_last_error()
    # the pooling's entries
    for f in (lib.fcl_hsd_pool_fwd, lib.fcl_hsd_pool_dx):
        assert f(256, 256, 256, None, 2, 100, 52, None) == -1 and f(None, 256, 256, 256, 2, 100, 52, None) == -1 and b"null" in lib.fcl_last_error()
        for n_utt, rows_in, rows_out in ((0, 100, 52), (2, 0, 1), (2, 2 ** 31, 52), (2, 100, 1), (2, 100, 53), (3, 2, 3)):
            assert f(256, 256, 256, 256, n_utt, rows_in, rows_out, None) == -2 and b"n_utt" in lib.fcl_last_error(), (n_utt, rows_in, rows_out)
    # the ctypes mirror is laid out like the header's struct
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fcl_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(fcl_hsd_t), '
                   'offsetof(fcl_hsd_t, groups), offsetof(fcl_hsd_t, slope), offsetof(fcl_hsd_t, src), offsetof(fcl_hsd_t, extra), '
                   'offsetof(fcl_hsd_t, workspace_bytes)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    L = _lib.HsdLayer
    assert out == [C.sizeof(L), L.groups.offset, L.slope.offset, L.src.offset, L.extra.offset, L.workspace_bytes.offset]
