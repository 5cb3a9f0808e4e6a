"""CPU checks for the trainable Parallel WaveGAN generator: the float64 numpy statement of tests/pwgt_ref.py against
oracle/pwg_oracle.generator_forward under torch autograd, a float32 evaluation inside its bounds, the mutants the bounds must reject, the saturation of
the gate in the arrays the GPU tests use, the construction-time refusals, the parameter names, the weight-norm fold, PWGPlan's acceptance of the module's
state dict and the argument validation of the fcl_pwt_* entries (which returns before any HIP call)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import pwgt_ref as R
from conftest import ROOT


@functools.lru_cache(maxsize=None)
def small():
    """the 4-layer stack on the packed batch: computed once and shared, read-only"""
    cfg = R.SMALL_STACK
    sd, ws, x0, c, ds = R.stack_case(cfg, 31)
    dils = R.dilations(cfg)
    fw = R.stack_forward(ws, x0, c, R.LENS, dils)
    bw = R.stack_backward(ws, fw, c, ds, R.LENS, dils)
    return cfg, sd, ws, x0, c, ds, dils, fw, bw


@pytest.fixture(scope="module")
def G():
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import pwg_generator

    return pwg_generator


def test_numpy_statement_agrees_with_the_oracle_under_autograd():
    cfg, sd, ws, x0, c, ds, dils, fw, bw = small()
    ts = R.torch_statement(sd, cfg, x0, c, ds, R.LENS)
    rel = lambda a, b: np.abs(a - b).max() / np.abs(b).max()
    worst = max([rel(fw["skips"], ts["skips"]), rel(bw["dx0"], ts["dx0"]), rel(bw["dc"], ts["dc"])] +
                [rel(fw["blocks"][l]["x_out"], ts["taps"][l]) for l in range(cfg["layers"])])
    from fcl_taco2_amd.pwg_generator import BLOCK_PARAMS

    last = cfg["layers"] - 1
    for l in range(cfg["layers"]):
        for name, got in zip(BLOCK_PARAMS, bw["grads"][l]):
            want = ts["grads"]["conv_layers.%d.%s" % (l, name)]
            if l == last and name.startswith("conv1x1_out"):
                assert not want.any() and not got.any()  # nobody reads the last block's x_out
            else:
                worst = max(worst, rel(got, want))
    assert worst <= 1e-12, worst


def test_float32_evaluation_stays_inside_every_bound():
    cfg, sd, ws, x0, c, ds, dils, fw, bw = small()
    with np.errstate(over="ignore"):
        f32 = R.stack_forward(ws, x0, c, R.LENS, dils, dt=np.float32)
        b32 = R.stack_backward(ws, f32, c, ds, R.LENS, dils, dt=np.float32)
    assert f32["skips"].dtype == np.float32 and b32["dx0"].dtype == np.float32
    inside = lambda got, want, e: bool((np.abs(got.astype(np.float64) - want) <= e).all())
    assert inside(f32["skips"], fw["skips"], fw["e_s"])
    for l in range(cfg["layers"]):
        a, b = f32["blocks"][l], fw["blocks"][l]
        assert inside(a["x_out"], b["x_out"], b["e_xout"]) and inside(a["a"], b["a"], b["e_a"]) and inside(a["b"], b["b"], b["e_b"])
        for got, want, e in zip(b32["grads"][l], bw["grads"][l], bw["e_grads"][l]):
            assert inside(got, want, e)
    assert inside(b32["dx0"], bw["dx0"], bw["e_dx0"]) and inside(b32["dc"], bw["dc"], bw["e_dc"])


def violates(mutant):
    cfg, sd, ws, x0, c, ds, dils, fw, bw = small()
    out = lambda got, want, e: bool((np.abs(got - want) > e).any())
    if mutant in R.MUTANTS_FWD:
        fm = R.stack_forward(ws, x0, c, R.LENS, dils, mutant)
        return out(fm["skips"], fw["skips"], fw["e_s"]) or any(out(m["x_out"], b["x_out"], b["e_xout"]) for m, b in zip(fm["blocks"], fw["blocks"]))
    bw = R.stack_backward(ws, fw, c, ds, R.LENS, dils, running=False)  # the first terms: what one launch may differ by on given inputs
    bm = R.stack_backward(ws, fw, c, ds, R.LENS, dils, running=False, mutant=mutant)
    bad = out(bm["dx0"], bw["dx0"], bw["e_dx0"]) or out(bm["dc"], bw["dc"], bw["e_dc"])
    return bad or any(out(g, w, e) for l in range(cfg["layers"]) for g, w, e in zip(bm["grads"][l], bw["grads"][l], bw["e_grads"][l]))


@pytest.mark.parametrize("mutant", R.MUTANTS_FWD + R.MUTANTS_BWD)
def test_mutants_leave_their_bound(mutant):
    assert violates(mutant), mutant


def test_the_unmutated_statement_is_inside_its_own_bounds():
    cfg, sd, ws, x0, c, ds, dils, fw, bw = small()
    again = R.stack_backward(ws, fw, c, ds, R.LENS, dils, running=False)
    assert np.array_equal(again["dx0"], bw["dx0"]) and (again["e_dx0"] <= bw["e_dx0"]).all()  # the first term is part of the running bound


def test_the_arrays_of_the_gpu_tests_saturate_the_gate():
    """at least 5 % of the tanh arguments beyond +-5 in every block-level cell and in every block of the small stack: otherwise 1 - a^2 and b (1 - b) are
    never small and the backward pass's differences near saturation go untested"""
    for name in R.BLOCK_CONFIGS:
        for d in R.DILATIONS:
            w, inp = R.block_case(name, d)
            z = R.gate_forward(w, inp["x"], inp["c"], R.LENS, d)["z"]
            Rc = inp["x"].shape[1]
            assert (np.abs(z[:, :Rc]) > 5).mean() >= 0.05, (name, d)
    cfg, sd, ws, x0, c, ds, dils, fw, bw = small()
    for blk in fw["blocks"]:
        assert (np.abs(blk["z"][:, : cfg["residual_channels"]]) > 5).mean() >= 0.05


def test_refusals_name_the_argument(G):
    bad = dict(in_channels=2, out_channels=2, kernel_size=7, layers=61, stacks=4, residual_channels=80, gate_channels=64, skip_channels=32,
               aux_channels=72, aux_context_window=-1, dropout=0.1, bias=False, use_weight_norm=None, use_causal_conv=True,
               upsample_conditional_features=False, upsample_net="UpsampleNetwork", upsample_params={"upsample_scales": [4], "freq_axis_kernel_size": 3})
    for name, value in bad.items():
        with pytest.raises(ValueError, match=r"PWG generator: %s=" % name):
            G.check_configuration(**{name: value})
        if name not in ("use_weight_norm",):
            with pytest.raises(ValueError, match=name):
                G.TrainableParallelWaveGANGenerator(**{name: value})
    for ok in (dict(residual_channels=16, gate_channels=32, skip_channels=16, aux_channels=128, kernel_size=5, layers=60, stacks=2), dict(layers=1, stacks=1)):
        assert len(G.check_configuration(**ok)) == ok["layers"]
    assert G.check_configuration() == [2 ** (l % 10) for l in range(30)]
    with pytest.raises(Exception, match="GPU device"):
        G.GeneratorPlan("cpu")


SMALL_ARGS = dict(layers=4, stacks=2, residual_channels=16, gate_channels=32, skip_channels=16, aux_channels=16, upsample_params={"upsample_scales": [2, 3]})
SMALL_CFG = dict(layers=4, stacks=2, residual_channels=16, gate_channels=32, skip_channels=16, aux_channels=16, upsample_scales=(2, 3))


def test_state_dict_names_are_the_vocoders(G):
    from fcl_taco2_amd import vocoder

    m = G.TrainableParallelWaveGANGenerator(use_weight_norm=False)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == dict(vocoder.param_spec())
    m = G.TrainableParallelWaveGANGenerator(use_weight_norm=False, **SMALL_ARGS)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == dict(vocoder.param_spec(SMALL_CFG)) and m.cfg() == dict(vocoder.CONFIG, **SMALL_CFG)
    wn = G.TrainableParallelWaveGANGenerator(**SMALL_ARGS)
    want = set()
    for k in vocoder.param_spec(SMALL_CFG):
        want |= {k[:-6] + "weight_g", k[:-6] + "weight_v"} if k.endswith("weight") else {k}
    assert set(wn.state_dict()) == want


def test_weight_norm_fold_is_torchs_and_both_forms_load(G):
    torch.manual_seed(3)
    wn = G.TrainableParallelWaveGANGenerator(**SMALL_ARGS)
    for p in wn.parameters():
        p.data.normal_()
    for prefix, m in wn.convs():
        shape = m.weight_v.shape
        ref = (torch.nn.Conv2d(shape[1], shape[0], (1, shape[3]), bias=False) if len(shape) == 4 else torch.nn.Conv1d(shape[1], shape[0], shape[2], bias=False))
        ref = torch.nn.utils.weight_norm(ref)
        ref.weight_g.data.copy_(m.weight_g.data)
        ref.weight_v.data.copy_(m.weight_v.data)
        ref(torch.zeros((1, shape[1], 1, shape[3]) if len(shape) == 4 else (1, shape[1], shape[2])))  # (its weight is recomputed by the forward hook)
        assert torch.allclose(m.folded(), ref.weight, rtol=1e-6, atol=1e-7), prefix
    plain = G.TrainableParallelWaveGANGenerator(use_weight_norm=False, **SMALL_ARGS)
    plain.load_state_dict({"model": {"generator": wn.state_dict()}})  # a whole checkpoint, weight-norm names into a plain module
    for (_, a), (_, b) in zip(plain.convs(), wn.convs()):
        assert torch.equal(a.weight, b.folded())
    back = G.TrainableParallelWaveGANGenerator(**SMALL_ARGS)
    back.load_state_dict(plain.state_dict())  # plain names into a weight-norm module
    for (_, a), (_, b) in zip(plain.convs(), back.convs()):
        assert torch.allclose(a.weight, b.folded(), rtol=1e-6, atol=1e-7)
    wn.remove_weight_norm()
    assert set(wn.state_dict()) == set(plain.state_dict()) and not wn.use_weight_norm
    for (_, a), (_, b) in zip(plain.convs(), wn.convs()):
        assert torch.equal(a.weight, b.weight)


@pytest.mark.parametrize("weight_norm", [False, True])
def test_pwgplan_accepts_the_modules_state_dict(G, weight_norm):
    """PWGPlan's own acceptance rule (fold, then every name of param_spec with its shape), without a device"""
    from fcl_taco2_amd import vocoder

    sd = vocoder.fold_weight_norm(G.TrainableParallelWaveGANGenerator(use_weight_norm=weight_norm).state_dict())
    for k, shp in vocoder.param_spec().items():
        assert k in sd and tuple(np.shape(sd[k])) == tuple(shp), k
    assert set(sd) == set(vocoder.param_spec())


def test_c_entries_validate_without_a_gpu(tmp_path):
    import __graft_entry__ as ge

    ge.build()
    from fcl_taco2_amd import _lib

    lib = _lib.load()
    entries = (lib.fcl_pwt_block_fwd, lib.fcl_pwt_block_dx, lib.fcl_pwt_block_dw)
    for f in entries:
        assert f(None, None) == -1 and b"null" in lib.fcl_last_error()
    pointers = [n for n, t in _lib.PwtBlock._fields_ if t is C.c_void_p]

    def block(**kw):
        a = _lib.PwtBlock()
        a.samples, a.residual, a.aux, a.ksize, a.dilation = 100, 64, 80, 3, 2
        for n in pointers:
            setattr(a, n, 256)
        a.workspace_bytes = 1 << 30
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    assert len(pointers) == 25
    for f in entries:
        for bad in (dict(residual=60), dict(residual=80), dict(residual=8), dict(aux=72), dict(aux=144), dict(aux=0)):
            assert f(C.byref(block(**bad)), None) == -2 and b"multiple of 16" in lib.fcl_last_error(), bad
        for k in (1, 2, 4, 7):
            assert f(C.byref(block(ksize=k)), None) == -2 and b"kernel size" in lib.fcl_last_error()
        assert f(C.byref(block(dilation=0)), None) == -2 and b"dilation" in lib.fcl_last_error()
        assert f(C.byref(block(samples=0)), None) == -2 and f(C.byref(block(samples=2 ** 31)), None) == -2
        assert f(C.byref(block(seg_lo=None)), None) == -1 and f(C.byref(block(seg_hi=None)), None) == -1
    fwd, dx, dw = entries
    for n in ("x", "c", "w_gate", "b_gate", "w_out", "b_out", "ab", "x_out", "skips"):
        assert fwd(C.byref(block(**{n: None})), None) == -1, n
    for n in ("x", "c", "w_gate", "w_out", "ab", "x_out", "skips", "z_out"):
        assert fwd(C.byref(block(**{n: 260})), None) == -3 and b"16-byte" in lib.fcl_last_error(), n
    for n in ("ds", "ab", "w_dz", "dz", "dxo"):
        assert dx(C.byref(block(**{n: None})), None) == -1, n
    assert dx(C.byref(block(last=1)), None) == -1 and b"but the last" in lib.fcl_last_error()  # the last block has no dxo
    assert dx(C.byref(block(w_dx=None)), None) == -1 and dx(C.byref(block(w_dc=None)), None) == -1
    for n in ("ds", "dxo", "ab", "w_dz", "w_dx", "w_dc", "dz", "dx", "dc"):
        assert dx(C.byref(block(**{n: 264})), None) == -3, n
    for n in ("x", "c", "ab", "dz", "ds", "dw_gate", "db_gate", "dw_out", "db_out", "workspace", "dxo"):
        assert dw(C.byref(block(**{n: None})), None) == -1, n
    assert dw(C.byref(block(x=260)), None) == -3
    need = lib.fcl_pwt_dw_workspace_bytes(100, 64, 80, 3)
    assert need == 1 * (3 * 64 + 80 + 1) * 128 * 4 and lib.fcl_pwt_dw_workspace_bytes(1025, 16, 16, 5) == 2 * (5 * 16 + 16 + 1) * 32 * 4
    assert lib.fcl_pwt_dw_workspace_bytes(0, 64, 80, 3) == 0
    assert dw(C.byref(block(workspace_bytes=need - 4)), None) == -5 and b"workspace" in lib.fcl_last_error()
    # the ctypes mirror is laid out like the header's struct
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fcl_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(fcl_pwt_t), '
                   'offsetof(fcl_pwt_t, seg_lo), offsetof(fcl_pwt_t, dxo), offsetof(fcl_pwt_t, workspace), offsetof(fcl_pwt_t, workspace_bytes)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    T = _lib.PwtBlock
    assert out == [C.sizeof(T), T.seg_lo.offset, T.dxo.offset, T.workspace.offset, T.workspace_bytes.offset]
