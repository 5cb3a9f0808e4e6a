"""The float64 statement of the HiFi-GAN period discriminator (tests/hfgd_ref.py) against torch, its bounds against a float32 evaluation
and against mutants, and everything of fcl_taco2_amd/hifigan_discriminator.py that needs no GPU: the refusals, the names, the weight-norm fold, the row
tables, the losses, the C entries' argument checks.

Gain: the chained cases run at hfgd_ref.GAIN = 1/4 of the Kaiming scale.  On exactly the GPU test's arrays (SMALL, lengths 11, 130, 1100, 77, 401) the
share of unsure mask cells per map is at most 0.68 % (the last map of period 3; the first three maps stay below 0.03 %), below the cap of 1 %, and no
gradient's bound exceeds its peak (the worst: 0.72 of it), so the gain was not halved.  The multi-period case (three layers, see hfgd_ref.MPD_CFG) has at
most 0.60 % unsure cells in a map, mask and L1 kinks together."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import hfgd_ref as R
from conftest import ROOT


@pytest.fixture(scope="module")
def P():
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import hifigan_discriminator

    return hifigan_discriminator


@functools.lru_cache(maxsize=None)
def case(p):
    return R.period_case(p)


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def share(diff, bound):
    return float(np.max(np.abs(diff) / np.maximum(bound, 1e-300)))


@pytest.mark.parametrize("p", R.PERIODS)
def test_numpy_statement_agrees_with_the_torch_statement(p):
    c = case(p)
    ts = R.torch_statement(c["cfg"], c["ws"], c["xs"], p, c["ds"], c["ex"])
    for r, th in zip(c["fw"], ts["h"]):
        assert [a.shape for a in r["h"]] == [b.shape for b in th]
        assert max(rel(a, b) for a, b in zip(r["h"], th)) <= 1e-12
    bw = c["bw"]
    assert max(rel(a, b) for a, b in zip(bw["gx"], ts["gx"])) <= 1e-12
    assert max(rel(a, b) for a, b in zip(bw["dw"], ts["dw"])) <= 1e-12 and max(rel(a, b) for a, b in zip(bw["db"], ts["db"])) <= 1e-12
    # without the direct feature-map gradients
    plain = R.period_backward(c["cfg"], c["ws"], c["xs"], c["fw"], c["ds"], p)
    tp = R.torch_statement(c["cfg"], c["ws"], c["xs"], p, c["ds"])
    assert max(rel(a, b) for a, b in zip(plain["gx"], tp["gx"])) <= 1e-12 and max(rel(a, b) for a, b in zip(plain["dw"], tp["dw"])) <= 1e-12
    assert max(rel(a, b) for a, b in zip(plain["db"], tp["db"])) <= 1e-12 and rel(plain["gx"][2], bw["gx"][2]) > 1e-3


@pytest.mark.parametrize("p", (2, 5))
def test_weight_norm_gradients_agree_with_torch(p):
    c = case(p)
    rng = np.random.default_rng(p)
    vg = [(W, np.sqrt((W ** 2).sum((1, 2))) * (0.8 + 0.4 * rng.random(W.shape[0]))) for W, _ in c["ws"]]
    ws = [(R.fold_weight(v, g), b) for (v, g), (_, b) in zip(vg, c["ws"])]
    xs = c["xs"][:3]
    fw = R.forward(c["cfg"], ws, xs, p)
    ds, ex = R.given_gradients(fw, p)
    bw = R.period_backward(c["cfg"], ws, xs, fw, ds, p, extras=ex)
    ts = R.torch_statement(c["cfg"], ws, xs, p, ds, ex, weight_norm=vg)
    assert max(rel(a, b) for a, b in zip(bw["gx"], ts["gx"])) <= 1e-12
    for l, (v, g) in enumerate(vg):
        dg, dv = R.weight_norm_gradients(v, g, bw["dw"][l])
        assert rel(dg, ts["dg"][l]) <= 1e-12 and rel(dv, ts["dv"][l]) <= 1e-12 and rel(bw["db"][l], ts["db"][l]) <= 1e-12


def test_the_three_losses_agree_with_torch():
    m = R.mpd_case()
    ref, cfg = m["ref"], m["cfg"]
    outs_r, outs_f = [], []
    for ws, p in zip(m["wss"], R.PERIODS):
        pr, pf = R.torch_statement(cfg, ws, m["real"], p), R.forward(cfg, ws, m["fake"], p)
        L = len(ws)
        outs_r.append([torch.tensor(np.concatenate([h[l].reshape(-1) for h in pr["h"]])) for l in range(L)])
        outs_f.append([torch.tensor(np.concatenate([r["h"][l].reshape(-1) for r in pf]), requires_grad=True) for l in range(L)])
    adv, fm, d_real, d_fake = R.torch_losses(outs_r, outs_f)
    for got, key in ((adv, "adv"), (fm, "fm"), (d_real, "d_real"), (d_fake, "d_fake")):
        assert abs(got.item() - ref[key]) <= 1e-12 * abs(ref[key]) and ref[key + "_e"] > 0
    # the whole generator gradient against autograd through the torch statement of every period
    xs = [torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in m["fake"]]
    import torch.nn.functional as F

    total = 0.0
    for ws, p, o_r in zip(m["wss"], R.PERIODS, outs_r):
        geo = R.geometry(cfg)
        maps = [[] for _ in geo]
        for x in xs:
            h = x[None, None, :]
            h = F.pad(h, (0, p - len(x) % p), "reflect") if len(x) % p else h
            h = h.view(1, 1, -1, p)
            for l, (ci, co, k, s, pad) in enumerate(geo):
                h = F.conv2d(h, torch.tensor(ws[l][0][..., None]), torch.tensor(ws[l][1]), stride=(s, 1), padding=(pad, 0))
                h = F.leaky_relu(h, cfg["negative_slope"]) if l < len(geo) - 1 else h
                maps[l].append(h[0].permute(2, 1, 0).reshape(-1))
        o_f = [torch.cat(v) for v in maps]
        a, f, _, _ = R.torch_losses([o_r], [o_f])
        total = total + (a + 2.0 * f) / len(R.PERIODS)
    total.backward()
    assert max(rel(g, x.grad.numpy()) for g, x in zip(ref["gx"], xs)) <= 1e-12
    assert ref["unsure"] <= R.CAP
    assert max(np.linalg.norm(e) / np.linalg.norm(g) for e, g in zip(ref["gx_e"], ref["gx"])) < 1.0


def to32(a):
    return None if a is None else np.asarray(a, dtype=np.float32)


@pytest.mark.parametrize("p", R.PERIODS)
def test_a_float32_evaluation_stays_inside_every_bound_and_the_cap_holds_per_array(p):
    """on exactly the GPU test's arrays: the unsure share of every map at most CAP, no gradient bound above its peak, and the statement itself evaluated in
    float32 (masks from its own float32 activations, as the device's) inside the running bounds"""
    c = case(p)
    shares = R.unsure_shares(c["fw"])
    bw = c["bw"]
    print("period %d at gain %g: unsure share per map %s, gradient bound / peak %s" % (p, R.GAIN, np.round(shares, 5), np.round(
        [b / k for b, k in zip(bw["g_bound"], bw["g_peak"])], 3)))
    assert max(shares) <= R.CAP
    assert all(b <= k for b, k in zip(bw["g_bound"], bw["g_peak"]))
    assert all(e.max() <= np.abs(d).max() for e, d in zip(bw["dw_e"], bw["dw"])) and all(e.max() <= np.abs(g).max() for e, g in zip(bw["gx_e"], bw["gx"]))
    ws32 = [(to32(W), to32(b)) for W, b in c["ws"]]
    xs32 = [to32(x) for x in c["xs"]]
    fw32 = R.forward(c["cfg"], ws32, xs32, p)
    for r, q in zip(c["fw"], fw32):
        assert all(a.dtype == np.float32 for a in q["h"])
        assert max(share(a.astype(np.float64) - b, e) for a, b, e in zip(q["h"], r["h"], r["e"])) <= 1.0
    b32 = R.period_backward(c["cfg"], ws32, xs32, fw32, [to32(d) for d in c["ds"]], p, extras=[[to32(e) for e in ex] for ex in c["ex"]])
    assert b32["dw"][2].dtype == np.float32
    assert max(share(np.linalg.norm(a - b), np.linalg.norm(e)) for a, b, e in zip(b32["gx"], bw["gx"], bw["gx_e"])) <= 1.0
    for key in ("dw", "db"):
        assert max(share(a.astype(np.float64) - b, e) for a, b, e in zip(b32[key], bw[key], bw[key + "_e"])) <= 1.0, key


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_violates_a_bound(mutant):
    p = 3
    c = case(p)
    cfg, ws, xs, fw, bw = c["cfg"], c["ws"], c["xs"], c["fw"], c["bw"]
    worst = 0.0
    if mutant in ("stride_plus_one", "score_three_taps"):  # the shapes differ already
        mf = R.forward(cfg, ws, xs, p, mutant)
        assert any(a["h"][-1].shape != b["h"][-1].shape for a, b in zip(mf, fw))
        return
    if mutant in ("across_boundary", "time_major", "zero_pad"):
        mf = R.forward(cfg, ws, xs, p, mutant)
        worst = max(share(a - b, e) for q, r in zip(mf, fw) for a, b, e in zip(q["h"], r["h"], r["e"]))
    if mutant == "slope_one_at_zero":  # needs activations that are exactly zero: a given-input layer
        hin = R.normal((p, 9, 16), 1)
        hin[:, ::2] = 0.0
        W, g = ws[1][0], R.normal((p, 3, 64), 2)
        want, e = R.layer_dx(W, g, hin, None, 3, 2, 0.1)
        worst = share(R.layer_dx(W, g, hin, None, 3, 2, 0.1, mutant=mutant)[0] - want, e)
    elif mutant not in ("across_boundary",):
        mb = R.period_backward(cfg, ws, xs, fw, c["ds"], p, extras=c["ex"], mutant=mutant)
        worst = max([worst] + [share(np.linalg.norm(a - b), np.linalg.norm(e)) for a, b, e in zip(mb["gx"], bw["gx"], bw["gx_e"])] +
                    [share(a - b, e) for key in ("dw", "db") for a, b, e in zip(mb[key], bw[key], bw[key + "_e"])])
    assert worst > 1.0, (mutant, worst)


def test_fold_is_the_reflection_pad_and_the_period_view():
    x = np.arange(11.0)
    seg = R.fold(x, 4)[:, :, 0]  # 11 -> 12 samples: x_pad[11] = x[9]
    assert seg.shape == (4, 3) and seg[3].tolist() == [3.0, 7.0, 9.0] and seg[0].tolist() == [0.0, 4.0, 8.0]
    g = np.ones((4, 3, 1))
    assert R.unfold_adjoint(g, 11, 4).tolist() == [1.0] * 9 + [2.0, 1.0]  # the reflected sample's double contribution


def test_check_configuration_refuses_each_unsupported_argument_by_name(P):
    assert P.check_configuration() == [(1, 32, 5, 3, 2), (32, 128, 5, 3, 2), (128, 512, 5, 3, 2), (512, 1024, 5, 3, 2), (1024, 1024, 5, 1, 2), (1024, 1, 2, 1, 1)]
    assert P.check_configuration(kernel_sizes=(3, 4), channels=16, max_downsample_channels=64, downsample_scales=(4, 2))[-2:] == [(16, 64, 3, 2, 1), (64, 1, 3, 1, 1)]
    assert P.check_configuration(**R.SMALL) == R.geometry(R.SMALL)
    bad = dict(in_channels=2, out_channels=2, period=17, kernel_sizes=(7, 3), channels=24, downsample_scales=(5,), max_downsample_channels=2048, bias=None,
               nonlinear_activation="ReLU", negative_slope=1.0, use_weight_norm="yes", use_spectral_norm=True)
    for name, value in bad.items():
        with pytest.raises(ValueError, match=name + "="):
            P.check_configuration(**{name: value})
    for more in (dict(period=0), dict(kernel_sizes=(5, 5)), dict(kernel_sizes=5), dict(channels=1040), dict(downsample_scales=()), dict(downsample_scales=(1,) * 9),
                 dict(downsample_scales=(0,)), dict(negative_slope=-0.1), dict(max_downsample_channels=8)):
        with pytest.raises(ValueError, match=list(more)[0] + "="):
            P.check_configuration(**more)
    with pytest.raises(ValueError, match="lens="):  # 2 samples under period 5: 3 to pad, only 1 to reflect
        P.check_configuration(period=5, lens=[100, 2])
    P.check_configuration(period=5, lens=[100, 4, 5])
    with pytest.raises(ValueError, match="use_spectral_norm=True"):
        P.HiFiGANPeriodDiscriminator(use_spectral_norm=True)
    with pytest.raises(ValueError, match="channels=100"):
        P.HiFiGANMultiPeriodDiscriminator(discriminator_params=dict(channels=100))
    from fcl_taco2_amd import _lib

    with pytest.raises(_lib.FclError, match="no CPU fallback"):
        P.HiFiGANMultiPeriodDiscriminator(discriminator_params=R.SMALL)(torch.zeros(2, 100))


def test_plan_geometry_and_kept_bytes(P):
    plan = P.PeriodPlan.__new__(P.PeriodPlan)
    plan.geometry, plan.period, plan.layers = P.check_configuration(**R.SMALL), 3, 6
    assert plan.heights(11) == [4, 2, 1, 1, 1, 1, 2] and plan.heights(1100) == [367, 123, 41, 14, 5, 5, 6]
    rows = plan.rows(R.LENS)
    per = [R.forward(R.SMALL, R.weights(R.SMALL, 0), [np.zeros(n)], 3)[0] for n in R.LENS]
    assert rows[0] == sum(r["x"].shape[0] * r["x"].shape[1] for r in per)
    assert rows[1:] == [sum(r["h"][l].shape[0] * r["h"][l].shape[1] for r in per) for l in range(6)]
    assert plan.act_shapes(rows) == [(rows[1], 16), (rows[2], 64), (rows[3], 64), (rows[4], 64), (rows[5], 64), (rows[6],)]
    assert plan.kept_bytes(R.LENS) == 4 * (rows[0] + 16 * rows[1] + 64 * sum(rows[2:6]))


def test_state_dict_names_shapes_and_round_trips(P):
    d = P.HiFiGANMultiPeriodDiscriminator()
    want = []
    for i in range(5):
        for l in range(5):
            want += ["discriminators.%d.convs.%d.0.%s" % (i, l, n) for n in ("weight_g", "weight_v", "bias")]
        want += ["discriminators.%d.output_conv.%s" % (i, n) for n in ("weight_g", "weight_v", "bias")]
    sd = d.state_dict()
    assert sorted(sd) == sorted(want) and [m.period for m in d.discriminators] == [2, 3, 5, 7, 11]
    assert sd["discriminators.0.convs.0.0.weight_v"].shape == (32, 1, 5, 1) and sd["discriminators.4.convs.3.0.weight_v"].shape == (1024, 512, 5, 1)
    assert sd["discriminators.2.convs.4.0.weight_v"].shape == (1024, 1024, 5, 1) and sd["discriminators.1.output_conv.weight_v"].shape == (1, 1024, 2, 1)
    assert sd["discriminators.1.convs.1.0.weight_g"].shape == (128, 1, 1, 1) and sd["discriminators.1.convs.1.0.bias"].shape == (128,)
    kw = dict(discriminator_params=dict(R.SMALL))
    plain = P.HiFiGANMultiPeriodDiscriminator(periods=(2, 3), discriminator_params=dict(R.SMALL, use_weight_norm=False, bias=False))
    assert sorted(plain.state_dict()) == sorted(["discriminators.%d.convs.%d.0.weight" % (i, l) for i in range(2) for l in range(5)] +
                                                ["discriminators.%d.output_conv.weight" % i for i in range(2)])
    # either form loads into either module, and so does a whole checkpoint
    a = P.HiFiGANMultiPeriodDiscriminator(**kw)
    b = P.HiFiGANMultiPeriodDiscriminator(discriminator_params=dict(R.SMALL, use_weight_norm=False))
    b.load_state_dict({"model": {"generator": {}, "discriminator": a.state_dict()}})
    for da, db in zip(a.discriminators, b.discriminators):
        for ma, mb in zip(da.conv_list(), db.conv_list()):
            assert torch.equal(ma.folded(), mb.weight)
    a2 = P.HiFiGANMultiPeriodDiscriminator(**kw)
    a2.load_state_dict(b.state_dict())
    for db, d2 in zip(b.discriminators, a2.discriminators):
        for mb, m2 in zip(db.conv_list(), d2.conv_list()):
            assert torch.allclose(m2.folded(), mb.weight, rtol=1e-6, atol=0)
    a.remove_weight_norm()
    assert sorted(a.state_dict()) == sorted(b.state_dict()) and all(torch.equal(a.state_dict()[k], b.state_dict()[k]) for k in b.state_dict())
    one = P.HiFiGANPeriodDiscriminator(period=7, **R.SMALL)
    one.load_state_dict(a2.discriminators[3].state_dict())
    assert torch.equal(one.output_conv.weight_v, a2.discriminators[3].output_conv.weight_v)


def test_weight_norm_fold_matches_torch(P):
    m = P.HiFiGANPeriodDiscriminator(**R.SMALL).double()
    with torch.no_grad():
        for c in m.conv_list():
            c.weight_g.mul_(torch.rand_like(c.weight_g) + 0.5)
    for c in m.conv_list():
        v, g = c.weight_v.detach(), c.weight_g.detach()
        conv = torch.nn.utils.weight_norm(torch.nn.Conv2d(v.shape[1], v.shape[0], (v.shape[2], 1)).double())
        with torch.no_grad():
            conv.weight_v.copy_(v), conv.weight_g.copy_(g)
        conv(torch.zeros(1, v.shape[1], v.shape[2], 1, dtype=torch.float64))  # the hook recomputes .weight
        want = conv.weight.detach().numpy()
        assert np.allclose(c.folded().detach().numpy(), want, rtol=1e-14, atol=0)
        assert np.allclose(R.fold_weight(v.numpy()[..., 0], g.numpy().reshape(-1)), want[..., 0], rtol=1e-14, atol=0)


def test_loss_helpers_and_layout_views(P):
    outs = [[torch.tensor([[1.0, 3.0]]), torch.tensor([0.5, 2.0])], [torch.tensor([[0.0, 0.0]]), torch.tensor([1.0, 1.0, 4.0])]]
    real = [[torch.tensor([[2.0, 1.0]]), torch.tensor([1.0, -1.0])], [torch.tensor([[1.0, -1.0]]), torch.tensor([0.0, 0.0, 1.0])]]
    assert float(P.generator_adversarial_loss(outs)) == pytest.approx(((0.25 + 1.0) / 2 + 9.0 / 3) / 2)
    r, f = P.discriminator_adversarial_loss(real, outs)
    assert float(r) == pytest.approx(((0.0 + 4.0) / 2 + 2.0 / 3) / 2) and float(f) == pytest.approx(((0.25 + 4.0) / 2 + 18.0 / 3) / 2)
    assert float(P.feature_match_loss(outs, real)) == pytest.approx(((1.0 + 2.0) / 2 + (1.0 + 1.0) / 2) / 2)
    a, b = P.split_batch([[torch.arange(8.0).reshape(4, 2), torch.arange(6.0)]])
    assert a[0][0].tolist() == [[0.0, 1.0], [2.0, 3.0]] and b[0][1].tolist() == [3.0, 4.0, 5.0]
    # the package's views of an equal-length batch: [B, C, H, p] and [B, H' p]
    B, p, H, Cc = 2, 3, 4, 5
    ref = torch.arange(float(B * Cc * H * p)).reshape(B, Cc, H, p)
    packed = ref.permute(0, 3, 2, 1).reshape(B * p * H, Cc)
    sc = torch.arange(float(B * (H + 1) * p)).reshape(B, H + 1, p)
    views = P.to_reference_layout([packed, sc.permute(0, 2, 1).reshape(-1)], p, B)
    assert torch.equal(views[0], ref) and torch.equal(views[1], sc.reshape(B, -1))


def test_c_entries_validate_without_a_gpu(tmp_path):
    import __graft_entry__ as ge

    ge.build()
    from fcl_taco2_amd import _lib

    lib = _lib.load()
    entries = (lib.fcl_hpd_layer_fwd, lib.fcl_hpd_layer_dx, lib.fcl_hpd_layer_dw)
    for f in entries:
        assert f(None, None) == -1 and b"null" in lib.fcl_last_error()

    def layer(**kw):
        a = _lib.HpdLayer()
        a.rows_in, a.rows_out, a.cin, a.cout, a.ksize, a.stride, a.pad, a.slope = 300, 100, 64, 128, 5, 3, 2, 0.1
        for n in ("src", "in_lo", "in_hi", "x", "w", "bias", "h", "g", "extra", "y", "dw", "db", "workspace"):
            setattr(a, n, 256)
        a.workspace_bytes = 1 << 30
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for f in entries:
        for bad in (dict(cin=60), dict(cout=1040), dict(cin=1, cout=1), dict(cin=2), dict(cin=8, cout=8), dict(cout=0)):
            assert f(C.byref(layer(**bad)), None) == -2 and b"multiples of 16" in lib.fcl_last_error(), bad
        for bad in (dict(ksize=4), dict(ksize=7), dict(stride=0), dict(stride=5), dict(pad=1), dict(cout=1), dict(cout=1, ksize=2, stride=2, pad=1),
                    dict(cout=1, ksize=4, stride=1, pad=1), dict(cin=1, ksize=2, stride=1, pad=1)):
            assert f(C.byref(layer(**bad)), None) == -2, bad
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
    assert dx(C.byref(layer(cin=1, extra=None)), None) == -1 and b"first layer" in lib.fcl_last_error()  # h has no meaning there
    assert dx(C.byref(layer(cin=1, h=None)), None) == -1
    assert dx(C.byref(layer(g=264)), None) == -3 and dx(C.byref(layer(extra=264)), None) == -3
    for n in ("x", "g", "dw", "workspace"):
        assert dw(C.byref(layer(**{n: None})), None) == -1
    need = lib.fcl_hpd_dw_workspace_bytes(100, 64, 128, 5)
    assert need == 1 * (5 * 64 + 1) * 128 * 4 and lib.fcl_hpd_dw_workspace_bytes(1025, 1, 16, 5) == 2 * 6 * 16 * 4
    assert lib.fcl_hpd_dw_workspace_bytes(1632, 1024, 1024, 5) == 2 * (5 * 1024 + 1) * 1024 * 4 and lib.fcl_hpd_dw_workspace_bytes(0, 64, 64, 3) == 0
    assert dw(C.byref(layer(workspace_bytes=need - 4)), None) == -5 and b"workspace" in lib.fcl_last_error()
    # the ctypes mirror is laid out like the header's struct
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fcl_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(fcl_hpd_t), '
                   'offsetof(fcl_hpd_t, slope), offsetof(fcl_hpd_t, src), offsetof(fcl_hpd_t, extra), offsetof(fcl_hpd_t, workspace_bytes)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    L = _lib.HpdLayer
    assert out == [C.sizeof(L), L.slope.offset, L.src.offset, L.extra.offset, L.workspace_bytes.offset]
