"""The float64 statement of the HiFi-GAN generator's training launches (tests/hfgt_ref.py) checked without a device: against
hifigan_ref's torch functions under float64 autograd, its bounds against float32 evaluations of exactly the arrays tests/test_gpu_hifigan_generator.py
runs, its mutants; and the module's refusals, names, state dicts and the C entries' argument checks."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hfgt_ref as R
import hifigan_ref as H
from conftest import ROOT

LENS = list(R.LENS)
F32 = np.float32


@functools.lru_cache(maxsize=None)
def small():
    sd, mel, dout = R.small_case()
    lens = list(H.GENERATOR_LENS)
    fw = R.generator_fwd(sd, R.SMALL, mel.astype(np.float64), lens)
    bw = R.generator_bwd(sd, R.SMALL, mel.astype(np.float64), lens, fw, dout.astype(np.float64))
    return sd, mel, dout, lens, fw, bw


@pytest.fixture(scope="module")
def G():
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import hifigan_generator

    return hifigan_generator


def split(a, lens):
    return np.split(a, np.cumsum(lens)[:-1])


def test_numpy_statement_agrees_with_hifigan_ref_under_float64_autograd():
    """the last stage's output, and the gradient of sum(out * dout) on its way back to every stage parameter, input_conv's parameters and the mel"""
    sd, mel, dout, lens, fw, bw = small()
    cfg = dict(R.SMALL, negative_slope=R.SLOPE)
    leaves = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in sd.items()}
    mels = [torch.tensor(m.astype(np.float64), requires_grad=True) for m in split(mel, lens)]
    hop = int(np.prod(cfg["upsample_scales"]))
    loss, outs = 0, []
    for m, d in zip(mels, split(dout, [n * hop for n in lens])):
        res = H.generator_f64(leaves, m, cfg)
        outs.append(res["stages"][-1])
        loss = loss + (res["stages"][-1] * torch.tensor(d.astype(np.float64))).sum()
    loss.backward()
    rel = lambda a, b: float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))
    assert rel(fw["out"], torch.cat(outs).detach().numpy()) < 1e-12
    for k, g in bw["grads"].items():
        assert rel(g, leaves[k].grad.numpy()) < 1e-12, k
    assert set(bw["grads"]) == set(sd) - {"output_conv.1.weight", "output_conv.1.bias"}
    assert rel(bw["dmel"], torch.cat([m.grad for m in mels]).numpy()) < 1e-12


def conv_shares(x, w, b, res, g, d, act, dt):
    """every convolution launch alone on given inputs, evaluated in dt -> the shares of the first-term bounds"""
    k = w.shape[2]
    x64, w64, b64, r64, g64 = (np.asarray(v, np.float64) for v in (x, w, b, res, g))
    out = []
    for rs in (None, r64):
        y, e = R.conv_fwd(x64, w64, b64, d, LENS, act=act, res=rs)
        out.append(R.share(R.conv_fwd(x64, w64, b64, d, LENS, act=act, res=rs, dt=dt)[0] - y, e))
    pre = np.asarray(res, np.float64)[:, ::-1][:, : w.shape[1]] if w.shape[1] <= w.shape[0] else None
    for p, cy in ((pre, None), (pre, x64[::-1].copy()), (None, None)):
        v, e, _ = R.conv_dx(g64, w64, d, LENS, pre=p, carry=cy)
        out.append(R.share(R.conv_dx(g64, w64, d, LENS, pre=p, carry=cy, dt=dt)[0] - v, e))
    want, got = R.conv_dw(x64, g64, k, d, LENS, act=act), R.conv_dw(x64, g64, k, d, LENS, act=act, dt=dt)
    return out + [R.share(got[0] - want[0], want[2]), R.share(got[1] - want[1], want[3])]


@pytest.mark.parametrize("k,d,c", R.CONV_CELLS)
def test_float32_convolution_launches_stay_inside_their_bounds(k, d, c):
    x, w, b, res, g = R.conv_case(k, d, c)
    assert max(conv_shares(x, w, b, res, g, d, True, F32)) <= 1.0


def test_float32_input_conv_stays_inside_its_bounds():
    x, w, b, res, g = R.conv_case(7, 1, 80, 512)
    assert max(conv_shares(x, w, b, res, g, 1, False, F32)) <= 1.0


@pytest.mark.parametrize("s,cin,lens", R.TCONV_CELLS)
def test_float32_transposed_convolution_stays_inside_its_bounds_and_is_torchs(s, cin, lens):
    x, w, b = (np.asarray(v, np.float64) for v in H.tconv_case(H.SEEDS["tconv"], s, cin, lens))
    u, e_u = R.tconv_fwd(x, w, b, s, lens)
    ref = np.concatenate([H.tconv(H.lrelu(H.f64(xx), R.SLOPE), H.f64(w), H.f64(b), s).numpy() for xx in split(x, lens)])
    assert np.abs(u - ref).max() < 1e-12
    du = np.random.RandomState(s).standard_normal(u.shape)
    dc, e_dc, _ = R.tconv_dx(x, w, s, lens, du)
    dW, db, e_dW, e_db = R.tconv_dw(x, s, lens, du)
    xt = torch.tensor(x, requires_grad=True)
    wt, bt = torch.tensor(w, requires_grad=True), torch.tensor(b, requires_grad=True)
    tot = 0
    for xx, dd in zip(torch.split(xt, lens), split(du, [n * s for n in lens])):
        tot = tot + (H.tconv(H.lrelu(xx, R.SLOPE), wt, bt, s) * torch.tensor(dd)).sum()
    tot.backward()
    for got, want in ((dc, xt.grad), (dW, wt.grad), (db, bt.grad)):
        assert np.abs(got - want.numpy()).max() < 1e-11
    assert R.share(R.tconv_fwd(x, w, b, s, lens, dt=F32)[0] - u, e_u) <= 1.0
    assert R.share(R.tconv_dx(x, w, s, lens, du, dt=F32)[0] - dc, e_dc) <= 1.0
    g32 = R.tconv_dw(x, s, lens, du, dt=F32)
    assert R.share(g32[0] - dW, e_dW) <= 1.0 and R.share(g32[1] - db, e_db) <= 1.0


@pytest.mark.parametrize("k,d,c", R.UNIT_CELLS)
def test_float32_unit_stays_inside_the_running_bound(k, d, c):
    x, w1, b1, w2, b2, g = (np.asarray(v, np.float64) for v in H.unit_case(H.SEEDS["unit"], k, d, c, LENS))
    fw, f32 = R.unit_fwd(x, w1, b1, w2, b2, d, LENS), R.unit_fwd(x, w1, b1, w2, b2, d, LENS, dt=F32)
    assert R.share(f32["xt"] - fw["xt"], fw["e_xt"]) <= 1.0 and R.share(f32["xo"] - fw["xo"], fw["e_xo"]) <= 1.0
    # backward on the evaluation's own xt, as the GPU test runs it
    xt = f32["xt"].astype(np.float64)
    bw, b32 = R.unit_bwd(x, xt, w1, w2, d, LENS, g), R.unit_bwd(x, xt, w1, w2, d, LENS, g, dt=F32)
    assert max(R.share(b32[n] - bw[n], bw["e_" + n]) for n in ("dxt", "dx")) <= 1.0
    assert max(R.share(a - b, e) for a, b, e in zip(b32["grads"], bw["grads"], bw["e_grads"])) <= 1.0


def module_shares(fw, bw, fw_, bw_):
    out = {"c0": R.share(fw_["c0"] - fw["c0"], fw["e_c0"]), "dmel": R.share(bw_["dmel"] - bw["dmel"], bw["e_dmel"])}
    for i, (a, b) in enumerate(zip(fw_["stages"], fw["stages"])):
        out["u%d" % i], out["out%d" % i] = R.share(a["u"] - b["u"], b["e_u"]), R.share(a["out"] - b["out"], b["e_out"])
    for k in bw["grads"]:
        out[k] = R.share(bw_["grads"][k] - bw["grads"][k], bw["e_grads"][k])
    return out


def test_small_generator_meets_the_cap_and_its_bounds_are_not_vacuous():
    sd, mel, dout, lens, fw, bw = small()
    print("unsure mask cells: %.3g of an array at most" % bw["unsure"])
    assert bw["unsure"] <= R.MASK_CAP
    assert fw["e_out"].max() < np.abs(fw["out"]).max() and bw["e_dmel"].max() < np.abs(bw["dmel"]).max()
    for k, e in bw["e_grads"].items():
        assert e.max() < np.abs(bw["grads"][k]).max(), k


def test_float32_numpy_generator_stays_inside_the_running_bound():
    sd, mel, dout, lens, fw, bw = small()
    fw_ = R.generator_fwd(sd, R.SMALL, mel, lens, dt=F32)
    bw_ = R.generator_bwd(sd, R.SMALL, mel, lens, fw_, dout, dt=F32)
    shares = module_shares(fw, bw, fw_, bw_)
    print({k: round(v, 4) for k, v in shares.items()})
    assert max(shares.values()) <= 1.0


def test_float32_torch_eager_stays_inside_the_whole_module_bound():
    """hifigan_ref.TorchHiFiGAN's expressions in float32 under autograd, the parameters as leaves"""
    sd, mel, dout, lens, fw, bw = small()
    cfg, nk = R.SMALL, len(R.SMALL["resblock_kernel_sizes"])
    P = {k: torch.tensor(v, requires_grad=True) for k, v in sd.items()}
    mels = [torch.tensor(m, requires_grad=True) for m in split(mel, lens)]
    hop = int(np.prod(cfg["upsample_scales"]))
    outs, tot = [], 0
    for m, d in zip(mels, split(dout, [n * hop for n in lens])):
        c = F.conv1d(m.t().unsqueeze(0), P["input_conv.weight"], P["input_conv.bias"], padding=3)
        for i, s in enumerate(cfg["upsample_scales"]):
            c = F.conv_transpose1d(F.leaky_relu(c, R.SLOPE), P["upsamples.%d.1.weight" % i], P["upsamples.%d.1.bias" % i], stride=s, padding=s // 2 + s % 2,
                                   output_padding=s % 2)
            cs = None
            for j, kr in enumerate(cfg["resblock_kernel_sizes"]):
                x = c
                for dd, dil in enumerate(cfg["resblock_dilations"][j]):
                    p = "blocks.%d." % (i * nk + j)
                    xt = F.conv1d(F.leaky_relu(x, R.SLOPE), P[p + "convs1.%d.1.weight" % dd], P[p + "convs1.%d.1.bias" % dd], dilation=dil,
                                  padding=(kr - 1) // 2 * dil)
                    x = F.conv1d(F.leaky_relu(xt, R.SLOPE), P[p + "convs2.%d.1.weight" % dd], P[p + "convs2.%d.1.bias" % dd], padding=(kr - 1) // 2) + x
                cs = x if cs is None else cs + x
            c = cs / nk
        outs.append(c[0].t())
        tot = tot + (c[0].t() * torch.tensor(d)).sum()
    tot.backward()
    assert R.share(torch.cat(outs).detach().numpy() - fw["out"], fw["e_out"]) <= 1.0
    assert R.share(torch.cat([m.grad for m in mels]).numpy() - bw["dmel"], bw["e_dmel"]) <= 1.0
    for k in bw["grads"]:
        assert R.share(P[k].grad.numpy() - bw["grads"][k], bw["e_grads"][k]) <= 1.0, k


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutants_leave_their_bound(mutant):
    x, w1, b1, w2, b2, g = (np.asarray(v, np.float64) for v in H.unit_case(H.SEEDS["unit"], 7, 3, 64, LENS))
    if mutant in ("phase_off_by_one", "tconv_across_edge"):
        s, cin, lens = R.TCONV_CELLS[1]
        a, w, b = (np.asarray(v, np.float64) for v in H.tconv_case(H.SEEDS["tconv"], s, cin, lens))
        u, e = R.tconv_fwd(a, w, b, s, lens)
        assert R.share(R.tconv_fwd(a, w, b, s, lens, mutant=mutant)[0] - u, e) > 1.0
    elif mutant == "no_seed_scale":
        sd, mel, dout, lens, fw, bw = small()
        bad = R.generator_bwd(sd, R.SMALL, mel.astype(np.float64), lens, fw, dout.astype(np.float64), mutant=mutant)
        assert R.share(bad["dmel"] - bw["dmel"], bw["e_dmel"]) > 1.0
    elif mutant == "conv2_dilated":
        fw = R.unit_fwd(x, w1, b1, w2, b2, 3, LENS)
        assert R.share(R.unit_fwd(x, w1, b1, w2, b2, 3, LENS, mutant=mutant)["xo"] - fw["xo"], fw["e_xo"]) > 1.0
    else:
        xt = R.unit_fwd(x, w1, b1, w2, b2, 3, LENS)["xt"]
        bw, bad = R.unit_bwd(x, xt, w1, w2, 3, LENS, g), R.unit_bwd(x, xt, w1, w2, 3, LENS, g, mutant=mutant)
        if mutant == "missing_bias_gradient":
            assert R.share(bad["grads"][1] - bw["grads"][1], bw["e_grads"][1]) > 1.0 and R.share(bad["grads"][3] - bw["grads"][3], bw["e_grads"][3]) > 1.0
        else:
            assert R.share(bad["dx"] - bw["dx"], bw["e_dx"]) > 1.0


def test_check_training_refuses_by_name(G):
    from fcl_taco2_amd import hifigan

    ok = G.check_training(hifigan.config())
    assert ok["channels"] == 512
    for name, value in (("in_channels", 72), ("in_channels", 1024), ("out_channels", 0), ("channels", 1024), ("kernel_size", 9),
                        ("upsample_scales", (32, 8, 2, 2)), ("resblock_kernel_sizes", (3, 5, 7, 11, 3))):
        with pytest.raises(ValueError, match=r"HiFi-GAN generator: %s=" % name):
            G.check_training(dict(ok, **{name: value}))
    with pytest.raises(ValueError, match="in_channels"):
        G.TrainableHiFiGANGenerator(in_channels=72)
    with pytest.raises(Exception, match="GPU device"):
        G.TrainingPlan("cpu")


SMALL_ARGS = {k: v for k, v in R.SMALL.items() if k != "negative_slope"}


def test_parameter_names_are_param_specs_in_both_forms(G):
    from fcl_taco2_amd import hifigan

    m = G.TrainableHiFiGANGenerator(use_weight_norm=False)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == dict(hifigan.param_spec())
    m = G.TrainableHiFiGANGenerator(use_weight_norm=False, **SMALL_ARGS)
    spec = hifigan.param_spec(H.plan_cfg(R.SMALL))
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == dict(spec)
    wn = G.TrainableHiFiGANGenerator(**SMALL_ARGS)
    want = set()
    for k in spec:
        want |= {k[:-6] + "weight_g", k[:-6] + "weight_v"} if k.endswith("weight") else {k}
    assert set(wn.state_dict()) == want
    # weight norm's dim 0 is the input channel of a transposed convolution, as hifigan_ref.with_weight_norm has it
    assert tuple(wn.state_dict()["upsamples.0.1.weight_g"].shape) == (128, 1, 1)


def test_load_state_dict_round_trips(G):
    from fcl_taco2_amd import vocoder

    sd, _, _ = R.small_case()
    plain = G.TrainableHiFiGANGenerator(use_weight_norm=False, **SMALL_ARGS)
    plain.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    assert all(np.array_equal(v.numpy(), sd[k]) for k, v in plain.state_dict().items())
    wn_sd = H.with_weight_norm(sd, np.random.RandomState(1))
    wn = G.TrainableHiFiGANGenerator(**SMALL_ARGS)
    wn.load_state_dict({"model": {"generator": {k: torch.from_numpy(v) for k, v in wn_sd.items()}}})  # a whole checkpoint
    for (p, a), (_, b) in zip(plain._named_convs(), wn._named_convs()):
        assert torch.allclose(a.weight, b.folded(), rtol=1e-5, atol=1e-7), p
    plain2 = G.TrainableHiFiGANGenerator(use_weight_norm=False, **SMALL_ARGS)
    plain2.load_state_dict(wn.state_dict())  # weight-norm names into a plain module
    back = G.TrainableHiFiGANGenerator(**SMALL_ARGS)
    back.load_state_dict(plain.state_dict())  # plain names into a weight-norm module
    for (p, a), (_, b), (_, c) in zip(plain._named_convs(), plain2._named_convs(), back._named_convs()):
        assert torch.allclose(a.weight, b.weight, rtol=1e-5, atol=1e-7) and torch.allclose(a.weight, c.folded(), rtol=1e-5, atol=1e-7), p
    # the inference plan's own acceptance rule, without a device
    from fcl_taco2_amd import hifigan

    for m in (plain, wn):
        folded = vocoder.fold_weight_norm(m.state_dict())
        assert {k: tuple(np.shape(v)) for k, v in folded.items()} == dict(hifigan.param_spec(H.plan_cfg(R.SMALL)))
    wn.remove_weight_norm()
    assert set(wn.state_dict()) == set(plain.state_dict())


def test_pack_and_unpack_are_inverse_permutations(G):
    w = torch.randn(32, 48, 7)
    fwd, dx = G.pack_conv(w)
    assert torch.equal(fwd.permute(2, 1, 0), w) and torch.equal(dx, w.flip(2).permute(2, 0, 1))
    t = torch.randn(64, 32, 8)
    tf, tdx = G.pack_tconv(t, 4)
    assert tuple(tf.shape) == (4, 2, 64, 32) and torch.equal(tf[1, 0], t[:, :, 5]) and torch.equal(tf[1, 1], t[:, :, 1])
    assert torch.equal(G.unpack_dweights(tdx.permute(0, 2, 1).contiguous(), torch.zeros(32), [])[0], t)


def test_c_entries_validate_without_a_gpu(tmp_path):
    import __graft_entry__ as ge

    ge.build()
    from fcl_taco2_amd import _lib

    lib = _lib.load()
    convs, tconvs = (lib.fcl_hft_conv_fwd, lib.fcl_hft_conv_dx, lib.fcl_hft_conv_dw), (lib.fcl_hft_tconv_fwd, lib.fcl_hft_tconv_dx, lib.fcl_hft_tconv_dw)
    for f in convs + tconvs:
        assert f(None, None) == -1 and b"null" in lib.fcl_last_error()

    def filled(T, **kw):
        a = T()
        a.rows, a.cin, a.cout, a.slope = 100, 64, 32, 0.1
        if T is _lib.HftConv:
            a.ksize, a.dilation = 3, 2
        else:
            a.stride = 4
        for n, t in T._fields_:
            if t is C.c_void_p:
                setattr(a, n, 256)
        a.workspace_bytes = 1 << 30
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for fs, T in ((convs, _lib.HftConv), (tconvs, _lib.HftTconv)):
        for f in fs:
            for bad in (dict(cin=24), dict(cin=528), dict(cout=8), dict(cout=0)):
                assert f(C.byref(filled(T, **bad)), None) == -2 and b"multiple of 16" in lib.fcl_last_error(), bad
            assert f(C.byref(filled(T, rows=0)), None) == -2 and f(C.byref(filled(T, rows=2 ** 31)), None) == -2
            assert f(C.byref(filled(T, slope=1.0)), None) == -1 and f(C.byref(filled(T, slope=-0.1)), None) == -1 and b"slope" in lib.fcl_last_error()
            assert f(C.byref(filled(T, seg_lo=None)), None) == -1 and f(C.byref(filled(T, seg_hi=None)), None) == -1
    for f in convs:
        for k in (2, 4, 9, 13):
            assert f(C.byref(filled(_lib.HftConv, ksize=k)), None) == -2 and b"kernel size" in lib.fcl_last_error()
        assert f(C.byref(filled(_lib.HftConv, dilation=0)), None) == -2 and b"dilation" in lib.fcl_last_error()
    for f in tconvs:
        assert f(C.byref(filled(_lib.HftTconv, stride=1)), None) == -2 and f(C.byref(filled(_lib.HftTconv, stride=17)), None) == -2
        assert f(C.byref(filled(_lib.HftTconv, rows=2 ** 29)), None) == -2
    fwd, dx, dw = convs
    for n in ("x", "w", "bias", "y"):
        assert fwd(C.byref(filled(_lib.HftConv, **{n: None})), None) == -1, n
    for n in ("x", "w", "res", "y"):
        assert fwd(C.byref(filled(_lib.HftConv, **{n: 260})), None) == -3 and b"16-byte" in lib.fcl_last_error(), n
    for n in ("x", "w", "y"):
        assert dx(C.byref(filled(_lib.HftConv, **{n: None})), None) == -1, n
    assert dx(C.byref(filled(_lib.HftConv, pre=264)), None) == -3
    for n in ("x", "g", "dw", "db", "workspace"):
        assert dw(C.byref(filled(_lib.HftConv, **{n: None})), None) == -1, n
    assert dw(C.byref(filled(_lib.HftConv, g=260)), None) == -3
    need = lib.fcl_hft_workspace_bytes(100, 64, 32, 3, 1)
    assert need == 1 * (3 * 64 + 1) * 32 * 4 and lib.fcl_hft_workspace_bytes(1025, 16, 16, 5, 1) == 2 * (5 * 16 + 1) * 16 * 4
    assert dw(C.byref(filled(_lib.HftConv, workspace_bytes=need - 4)), None) == -5 and b"workspace" in lib.fcl_last_error()
    tf, tdx, tdw = tconvs
    for f, names in ((tf, ("c", "w", "bias", "u")), (tdx, ("c", "w", "du", "dc")), (tdw, ("c", "du", "dw", "db", "workspace"))):
        for n in names:
            assert f(C.byref(filled(_lib.HftTconv, **{n: None})), None) == -1, n
        assert f(C.byref(filled(_lib.HftTconv, c=260)), None) == -3
    need = lib.fcl_hft_workspace_bytes(100, 64, 32, 8, 4)  # partials of 1 024 / 4 input rows, 2 s taps and s bias rows
    assert need == 1 * (8 * 64 + 4) * 32 * 4 and lib.fcl_hft_workspace_bytes(257, 64, 32, 8, 4) == 2 * (8 * 64 + 4) * 32 * 4
    assert lib.fcl_hft_workspace_bytes(0, 64, 32, 3, 1) == 0
    assert tdw(C.byref(filled(_lib.HftTconv, workspace_bytes=need - 4)), None) == -5
    arr = (C.c_void_p * 2)(256, 512)
    assert lib.fcl_hft_sum(None, arr, 2, 1.0, 64, None) == -1 and lib.fcl_hft_sum(256, arr, 5, 1.0, 64, None) == -2
    assert lib.fcl_hft_sum(256, arr, 2, 1.0, 62, None) == -2 and lib.fcl_hft_sum(260, arr, 2, 1.0, 64, None) == -3
    # the ctypes mirrors are laid out like the header's structs
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fcl_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(fcl_hft_conv_t), offsetof(fcl_hft_conv_t, seg_lo), offsetof(fcl_hft_conv_t, workspace_bytes), sizeof(fcl_hft_tconv_t), '
                   'offsetof(fcl_hft_tconv_t, seg_lo), offsetof(fcl_hft_tconv_t, workspace_bytes)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    A, B = _lib.HftConv, _lib.HftTconv
    assert out == [C.sizeof(A), A.seg_lo.offset, A.workspace_bytes.offset, C.sizeof(B), B.seg_lo.offset, B.workspace_bytes.offset]
