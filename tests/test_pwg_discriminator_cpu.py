"""CPU checks for the Parallel WaveGAN discriminator: the float64 numpy statement of tests/pwgd_ref.py against its torch statement, the
mutants its bounds must reject, the near-kink condition of the recorded seeds, the construction-time refusals, the parameter names, the weight-norm fold
and the argument validation of the fcl_pwd_* entries (which returns before any HIP call)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import pwgd_ref as R
from conftest import ROOT


@functools.lru_cache(maxsize=None)
def case_data(name):
    """computed once per case and shared, read-only"""
    cfg, lens = R.CONFIGS[name], dict(R.CASES)[name]
    ws, xs, ds = R.weights(cfg, 0), R.signals(lens, 0), R.given_gradient(lens, 0)
    fw = R.forward(cfg, ws, xs)
    stored = [[h.astype(np.float32).astype(np.float64) for h in r["h"][:-1]] for r in fw]  # what a device would have kept
    bw = R.backward(cfg, ws, xs, stored, ds)
    return cfg, ws, xs, ds, fw, stored, bw


@pytest.fixture(scope="module")
def P():
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import pwg_discriminator

    return pwg_discriminator


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_numpy_statement_agrees_with_the_torch_statement(name):
    cfg, ws, xs, ds, fw, _, _ = case_data(name)
    bw = R.backward(cfg, ws, xs, [r["h"][:-1] for r in fw], ds)  # on its own float64 activations, as autograd does
    ts = R.torch_statement(cfg, ws, xs, ds)
    rel = lambda a, b: np.abs(a - b).max() / np.abs(b).max()
    worst = max(rel(fw[u]["h"][l], ts["h"][u][l]) for u in range(len(xs)) for l in range(cfg["layers"]))
    worst = max([worst] + [rel(a, b) for a, b in zip(bw["gx"], ts["gx"])] + [rel(a, b) for a, b in zip(bw["dw"], ts["dw"])])
    if cfg["bias"]:
        worst = max([worst] + [rel(a, b) for a, b in zip(bw["db"], ts["db"])])
    assert worst <= 1e-12, worst


def violates(name, mutant):
    """the mutant's results leave a bound of the reference somewhere in this case"""
    cfg, ws, xs, ds, fw, stored, bw = case_data(name)
    if mutant in ("dilation_plus_one", "across_boundary", "d_i_is_i_plus_1"):
        fm = R.forward(cfg, ws, xs, mutant)
        return any((np.abs(m - h) > e).any() for rm, r in zip(fm, fw) for m, h, e in zip(rm["h"], r["h"], r["e"]))
    bm = R.backward(cfg, ws, xs, stored, ds, mutant)
    out = any(np.linalg.norm(a - b) > np.linalg.norm(e) for a, b, e in zip(bm["gx"], bw["gx"], bw["gx_e"]))
    out = out or any((np.abs(a - b) > e).any() for a, b, e in zip(bm["dw"], bw["dw"], bw["dw_e"]))
    return out or any((np.abs(a - b) > e).any() for a, b, e in zip(bm["db"], bw["db"], bw["db_e"]))


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_violates_a_bound(mutant):
    hit = [name for name in R.CONFIGS if violates(name, mutant)]
    print(mutant, "rejected on", hit)
    assert hit


def test_the_statement_itself_meets_its_bounds_in_float32():
    """a float32 numpy evaluation of one case (another summation order than any kernel's) stays inside the forward bounds"""
    cfg, ws, xs, _, fw, _, _ = case_data("c16k5f2")
    geo = R.geometry(cfg)
    for x, r in zip(xs, fw):
        h = x[:, None].astype(np.float32)
        for l, ((W, b), (ci, co, d)) in enumerate(zip(ws, geo)):
            pre = np.zeros((len(x), co), np.float32)
            for j, s, t0, t1 in R._taps(W.shape[2], d, len(x)):
                pre[t0:t1] += h[t0 + s : t1 + s] @ W[:, :, j].T.astype(np.float32)
            pre += np.float32(0) if b is None else b.astype(np.float32)
            h = np.where(pre > 0, pre, np.float32(cfg["negative_slope"]) * pre).astype(np.float32) if l < len(geo) - 1 else pre
            assert (np.abs(h - r["h"][l]) <= r["e"][l]).all(), l


@pytest.mark.parametrize("loss", sorted(R.SEEDS))
def test_near_kink_condition_holds_for_the_recorded_seeds(loss):
    ref = R.e2e_reference(R.SEEDS[loss], loss)
    assert ref["share"] == 1.0
    assert R.first_clean_seed(loss) == R.SEEDS[loss]  # and it is the first clean one among the first 80


@pytest.mark.parametrize("loss", sorted(R.SEEDS))
def test_end_to_end_reference_agrees_with_torch_autograd(loss):
    """the adversarial losses and the weight-norm chain of e2e_reference against F.conv1d + autograd in float64"""
    import torch.nn.functional as F

    ref = R.e2e_reference(R.SEEDS[loss], loss)
    cfg, geo = ref["cfg"], R.geometry(ref["cfg"])
    leaf = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)
    vs, gs, bs = [leaf(v) for v in ref["vs"]], [leaf(g) for g in ref["gs"]], [leaf(b) for b in ref["bs"]]
    xs = [leaf(x) for x in ref["xs"]]
    scores = []
    for x in xs:
        h = x[None, None, :]
        for l, (ci, co, d) in enumerate(geo):
            w = vs[l] * (gs[l] / torch.linalg.vector_norm(vs[l], dim=(1, 2)))[:, None, None]
            h = F.conv1d(h, w, bs[l], dilation=d, padding=(cfg["kernel_size"] - 1) // 2 * d)
            h = F.leaky_relu(h, cfg["negative_slope"]) if l < len(geo) - 1 else h
        scores.append(h[0, 0])
    if loss == "generator":
        value = torch.mean((torch.cat(scores) - 1.0) ** 2)
    else:
        R_ = len(ref["real"])
        value = torch.mean((torch.cat(scores[:R_]) - 1.0) ** 2) + torch.mean(torch.cat(scores[R_:]) ** 2)
    value.backward()
    close = lambda a, b: np.allclose(a, b.grad.numpy(), rtol=1e-10, atol=1e-14)
    assert abs(value.item() - ref["value"]) <= 1e-12 * abs(ref["value"])
    assert all(close(a, b) for a, b in zip(ref["gx"], xs))
    assert all(close(a, b) for a, b in zip(ref["dg"], gs)) and all(close(a, b) for a, b in zip(ref["dv"], vs)) and all(close(a, b) for a, b in zip(ref["db"], bs))
    assert all((e > 0).all() for key in ("gx_e", "dg_e", "dv_e", "db_e") for e in ref[key])


def test_check_configuration_refuses_each_unsupported_argument_by_name(P):
    assert P.check_configuration() == [(1, 64, 1)] + [(64, 64, i) for i in range(1, 9)] + [(64, 1, 1)]
    assert 1 + 2 * sum(d for _, _, d in P.check_configuration()) == 77  # the receptive field of the defaults
    assert [d for _, _, d in P.check_configuration(dilation_factor=2, layers=5)] == [1, 2, 4, 8, 1]
    bad = dict(in_channels=2, out_channels=2, kernel_size=7, layers=2, conv_channels=72, dilation_factor=0, nonlinear_activation="ReLU",
               negative_slope=1.0, bias=None, use_weight_norm="yes")
    for name, value in bad.items():
        with pytest.raises(ValueError, match=name + "="):
            P.check_configuration(**{name: value})
    for more in (dict(kernel_size=4), dict(layers=17), dict(conv_channels=144), dict(conv_channels=8), dict(negative_slope=-0.1)):
        with pytest.raises(ValueError, match=list(more)[0] + "="):
            P.check_configuration(**more)
    with pytest.raises(ValueError, match="conv_channels=100"):
        P.ParallelWaveGANDiscriminator(conv_channels=100)
    from fcl_taco2_amd import _lib

    with pytest.raises(_lib.FclError, match="no CPU fallback"):
        P.ParallelWaveGANDiscriminator()(torch.zeros(2, 100))


def test_state_dict_names_and_initialisation(P):
    d = P.ParallelWaveGANDiscriminator()
    want = []
    for i in range(10):
        want += ["conv_layers.%d.weight_g" % (2 * i), "conv_layers.%d.weight_v" % (2 * i), "conv_layers.%d.bias" % (2 * i)]
    assert sorted(d.state_dict()) == sorted(want)
    sd = d.state_dict()
    assert sd["conv_layers.0.weight_v"].shape == (64, 1, 3) and sd["conv_layers.8.weight_v"].shape == (64, 64, 3) and sd["conv_layers.18.weight_v"].shape == (1, 64, 3)
    assert sd["conv_layers.4.weight_g"].shape == (64, 1, 1) and not any(bool(sd[k].any()) for k in sd if k.endswith("bias"))
    assert abs(float(sd["conv_layers.8.weight_v"].std()) / np.sqrt(2.0 / 192) - 1) < 0.05  # Kaiming normal: std sqrt(2 / fan_in)
    p = P.ParallelWaveGANDiscriminator(layers=4, conv_channels=16, bias=False, use_weight_norm=False)
    assert sorted(p.state_dict()) == ["conv_layers.%d.weight" % i for i in (0, 2, 4, 6)]
    # either form loads into either module, and so does a whole parallel_wavegan checkpoint
    a = P.ParallelWaveGANDiscriminator(layers=4, conv_channels=16)
    b = P.ParallelWaveGANDiscriminator(layers=4, conv_channels=16, use_weight_norm=False)
    b.load_state_dict({"model": {"generator": {}, "discriminator": a.state_dict()}})
    for ma, mb in zip(a.convs(), b.convs()):
        assert torch.equal(ma.folded(), mb.weight)
    a2 = P.ParallelWaveGANDiscriminator(layers=4, conv_channels=16)
    a2.load_state_dict(b.state_dict())
    for mb, m2 in zip(b.convs(), a2.convs()):
        assert torch.allclose(m2.folded(), mb.weight, rtol=1e-6, atol=0)
    a.remove_weight_norm()
    assert sorted(a.state_dict()) == sorted(b.state_dict()) and all(torch.equal(a.state_dict()[k], b.state_dict()[k]) for k in b.state_dict())


def test_weight_norm_fold_matches_torch(P):
    m = P.ParallelWaveGANDiscriminator(layers=3, conv_channels=32).double()
    with torch.no_grad():
        for c in m.convs():
            c.weight_g.mul_(torch.rand_like(c.weight_g) + 0.5)
    for c in m.convs():
        want = R.torch_weight_norm_statement(c.weight_v.detach().numpy(), c.weight_g.detach().numpy().reshape(-1))
        assert np.allclose(c.folded().detach().numpy(), want, rtol=1e-14, atol=0)
        assert np.allclose(R.fold(c.weight_v.detach().numpy(), c.weight_g.detach().numpy().reshape(-1)), want, rtol=1e-14, atol=0)


def test_adversarial_loss_helpers(P):
    p, q = torch.tensor([[0.5, 2.0]]), torch.tensor([[1.0, -1.0]])
    assert float(P.generator_adversarial_loss(p)) == pytest.approx((0.25 + 1.0) / 2)
    r, f = P.discriminator_adversarial_loss(p, q)
    assert float(r) == pytest.approx(0.625) and float(f) == pytest.approx(1.0)


def test_c_entries_validate_without_a_gpu(tmp_path):
    import __graft_entry__ as ge

    ge.build()
    from fcl_taco2_amd import _lib

    lib = _lib.load()
    entries = (lib.fcl_pwd_layer_fwd, lib.fcl_pwd_layer_dx, lib.fcl_pwd_layer_dw)
    for f in entries:
        assert f(None, None) == -1 and b"null" in lib.fcl_last_error()

    def layer(**kw):
        a = _lib.PwdLayer()
        a.samples, a.cin, a.cout, a.ksize, a.dilation, a.slope = 100, 64, 64, 3, 2, 0.2
        for n in ("x", "w", "bias", "h", "g", "seg_lo", "seg_hi", "y", "dw", "db", "workspace"):
            setattr(a, n, 256)
        a.workspace_bytes = 1 << 30
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for f in entries:
        for bad in (dict(cin=60, cout=60), dict(cin=144, cout=144), dict(cin=64, cout=32), dict(cin=1, cout=1), dict(cin=2, cout=64), dict(cin=8, cout=8)):
            assert f(C.byref(layer(**bad)), None) == -2 and b"multiple of 16" in lib.fcl_last_error(), bad
        for k in (1, 2, 4, 7):
            assert f(C.byref(layer(ksize=k)), None) == -2 and b"kernel size" in lib.fcl_last_error()
        assert f(C.byref(layer(dilation=0)), None) == -2 and b"dilation" in lib.fcl_last_error()
        assert f(C.byref(layer(samples=0)), None) == -2 and f(C.byref(layer(samples=2 ** 31)), None) == -2
        assert f(C.byref(layer(slope=1.0)), None) == -1 and b"negative_slope" in lib.fcl_last_error()
        assert f(C.byref(layer(seg_lo=None)), None) == -1 and f(C.byref(layer(seg_hi=None)), None) == -1
    fwd, dx, dw = entries
    for n in ("x", "w", "y"):
        assert fwd(C.byref(layer(**{n: None})), None) == -1
        assert fwd(C.byref(layer(**{n: 260})), None) == -3 and b"16-byte" in lib.fcl_last_error()
    for n in ("g", "w", "y", "h"):
        assert dx(C.byref(layer(**{n: None})), None) == -1
    assert dx(C.byref(layer(cin=1, cout=64)), None) == -1 and b"first layer" in lib.fcl_last_error()  # h has no meaning there
    assert dx(C.byref(layer(g=264)), None) == -3
    for n in ("x", "g", "dw", "workspace"):
        assert dw(C.byref(layer(**{n: None})), None) == -1
    need = lib.fcl_pwd_dw_workspace_bytes(100, 64, 64, 3)
    assert need == 1 * (3 * 64 + 1) * 64 * 4 and lib.fcl_pwd_dw_workspace_bytes(1025, 1, 16, 5) == 2 * 6 * 16 * 4
    assert lib.fcl_pwd_dw_workspace_bytes(0, 64, 64, 3) == 0
    assert dw(C.byref(layer(workspace_bytes=need - 4)), None) == -5 and b"workspace" in lib.fcl_last_error()
    # the ctypes mirror is laid out like the header's struct
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fcl_hip.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(fcl_pwd_t), '
                   'offsetof(fcl_pwd_t, x), offsetof(fcl_pwd_t, workspace_bytes)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [C.sizeof(_lib.PwdLayer), _lib.PwdLayer.x.offset, _lib.PwdLayer.workspace_bytes.offset]
