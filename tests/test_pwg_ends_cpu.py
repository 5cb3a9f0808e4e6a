"""CPU checks for the HIP ends of the trainable Parallel WaveGAN generator: the float64 numpy statement of tests/pwge_ref.py (composed with
pwgt_ref.py's residual stack) against oracle/pwg_oracle.upsample + generator_forward under torch autograd, a float32 evaluation inside every bound on
exactly the arrays the GPU tests use (with the cap on the cells the ReLU kinks leave out), the mutants the bounds must reject, the refusals by name, and
the argument validation of the fcl_pwe_* entries (which returns before any HIP call) with the struct's layout."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import helpers as H
import pwge_ref as E
import pwgt_ref as R
from conftest import ROOT


@pytest.fixture(scope="module")
def G():
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import pwg_generator

    return pwg_generator


def test_numpy_statement_agrees_with_the_oracle_under_autograd():
    """the whole generator: pwge_ref's ends around pwgt_ref's stack on a packed batch, against per-utterance float64 torch runs of the oracle"""
    from oracle import pwg_oracle as O

    frames, scales, ctx = (1, 2, 5), (2, 3), 2
    cfg = dict(R.SMALL_STACK, upsample_scales=scales, aux_context_window=ctx)
    Rc, A, L, hop = cfg["residual_channels"], cfg["aux_channels"], cfg["layers"], 6
    rng = np.random.RandomState(77)
    sd = {k: np.asarray(v, np.float64) for k, v in H.pwg_random_state_dict(rng, cfg, 1.0).items()}
    w, ws, dils = E.weights_of(sd, len(scales)), [R.block_weights(sd, l) for l in range(L)], R.dilations(cfg)
    lens, n = [f * hop for f in frames], sum(frames) * hop
    c, z, dwav = rng.standard_normal((sum(frames) + 2 * ctx * len(frames), A)), rng.standard_normal(n), rng.standard_normal(n)
    fi = E.input_forward(w, c, z, frames, scales, ctx)
    fs = R.stack_forward(ws, fi["x0"], fi["cu"], lens, dils, running=False)
    fo = E.output_forward(w, fs["skips"], L)
    bo = E.output_backward(w, fs["skips"], L, dwav, fo["p1"] > 0, fs["skips"] > 0, y1=fo["y1"])
    bs = R.stack_backward(ws, fs, fi["cu"], bo["ds"], lens, dils, running=False)
    bi = E.input_backward(w, c, z, fi, bs["dc"], bs["dx0"], frames, scales, ctx)
    t = {k: torch.tensor(v, requires_grad=True) for k, v in sd.items()}
    got = dict(cu=[], wav=[], dz=[], dc=[])
    for (lo, hi), (clo, chi) in zip(E.spans(frames, hop), E.spans(frames, extra=2 * ctx)):
        cb, zb = torch.tensor(c[clo:chi].T[None], requires_grad=True), torch.tensor(z[lo:hi][None, None], requires_grad=True)
        cu = O.upsample(t, cb, cfg)
        y = O.generator_forward(t, zb, cu, cfg)
        y.backward(torch.tensor(dwav[lo:hi][None, None]))
        got["cu"].append(cu[0].t().detach().numpy())
        got["wav"].append(y[0, 0].detach().numpy())
        got["dz"].append(zb.grad[0, 0].numpy())
        got["dc"].append(cb.grad[0].t().numpy())
    close = lambda a, b, what: np.testing.assert_allclose(a, b, rtol=0, atol=1e-12 * max(np.abs(b).max(), 1e-300), err_msg=what)
    close(fi["cu"], np.concatenate(got["cu"]), "cu")
    close(fo["wav"], np.concatenate(got["wav"]), "wav")
    close(bi["dz"], np.concatenate(got["dz"]), "dz")
    close(bi["dc"], np.concatenate(got["dc"]), "dc")
    g = lambda k: t[k].grad.numpy()
    close(bi["dwin"], g("upsample_net.conv_in.weight"), "conv_in")
    for i in range(len(scales)):
        close(bi["dhs"][i], g("upsample_net.upsample.up_layers.%d.weight" % (2 * i + 1)).reshape(-1), "filter %d" % i)
    close(bi["dw0"], g("first_conv.weight").reshape(-1), "first_conv.weight")
    close(bi["db0"], g("first_conv.bias"), "first_conv.bias")
    close(bo["dW1"], g("last_conv_layers.1.weight")[:, :, 0], "last 1 weight")
    close(bo["db1"], g("last_conv_layers.1.bias"), "last 1 bias")
    close(bo["dw3"], g("last_conv_layers.3.weight").reshape(-1), "last 3 weight")
    close(bo["db3"], g("last_conv_layers.3.bias"), "last 3 bias")


def test_whole_generator_bounds_hold_for_a_float32_torch_evaluation():
    """pwge_ref.generator (the ends around pwgt_ref's stack, every error carried through) on the batch the GPU test of the module uses: its float64
    values are the oracle's under autograd to 1e-12, and the oracle evaluated in float32 on the CPU stays inside its bounds, for the waveform and every
    parameter's gradient"""
    from oracle import pwg_oracle as O

    frames, hop = list(E.MODULE_FRAMES), 6
    cfg, sd, mels, noise, dwav = E.module_case()
    ctx = cfg["aux_context_window"]
    cp, zp, wav, e_wav, grads, bounds = E.module_reference()
    print("the waveform's bound: %.3g of the peak" % (e_wav.max() / np.abs(wav).max()))
    assert e_wav.max() <= 1e-2 * np.abs(wav).max()  # (a condition on the case: a bound near the peak would admit anything)
    assert set(grads) == set(sd)
    for dt, tol in ((torch.float64, None), (torch.float32, 1.0)):
        t = {k: torch.tensor(np.asarray(v), dtype=dt, requires_grad=True) for k, v in sd.items()}
        ys = []
        for (lo, hi), (clo, chi) in zip(E.spans(frames, hop), E.spans(frames, extra=2 * ctx)):
            y = O.generator_forward(t, torch.tensor(zp[lo:hi][None, None], dtype=dt), O.upsample(t, torch.tensor(cp[clo:chi].T[None], dtype=dt), cfg), cfg)
            y.backward(torch.tensor(dwav[lo:hi][None, None], dtype=dt))
            ys.append(y[0, 0].detach().numpy().astype(np.float64))
        got = np.concatenate(ys)
        dead = "conv_layers.%d.conv1x1_out" % (cfg["layers"] - 1)
        if tol is None:
            assert np.abs(got - wav).max() <= 1e-12 * np.abs(wav).max()
            for k in sd:
                gk = np.zeros(grads[k].shape) if t[k].grad is None else t[k].grad.numpy()
                assert np.abs(gk - grads[k]).max() <= 1e-12 * max(np.abs(grads[k]).max(), 1e-300), k
        else:
            shares = {"wav": E.share(got - wav, e_wav)}
            for k in sd:
                if not k.startswith(dead):
                    shares[k] = E.share(t[k].grad.numpy().astype(np.float64) - grads[k], bounds[k])
            print({k: round(v, 4) for k, v in shares.items()})
            assert max(shares.values()) <= tol, shares


@pytest.mark.parametrize("shape,A,ctx,Rc", E.CASES)
def test_float32_evaluation_stays_inside_every_bound(shape, A, ctx, Rc):
    """on exactly the arrays the GPU tests use; the cells the kink of a mask leaves out stay under the cap"""
    ref = E.reference(shape, A, ctx, Rc)
    w, inp, frames, scales, f4 = ref["w"], ref["inp"], ref["frames"], ref["scales"], np.float32
    fw = E.input_forward(w, inp["c"], inp["z"], frames, scales, ctx, dt=f4)
    bw = E.input_backward(w, inp["c"], inp["z"], fw, inp["dcu"], inp["dx0"], frames, scales, ctx, dt=f4)
    assert fw["cu"].dtype == f4 and bw["dhs"][0].dtype == f4 and bw["dwin"].dtype == f4
    rf, rb = ref["fw"], ref["bw"]
    shares = {"cu": E.share(fw["cu"] - rf["cu"], rf["e_cu"]), "x0": E.share(fw["x0"] - rf["x0"], rf["e_x0"])}
    for i in range(len(scales)):
        shares["u%d" % i] = E.share(fw["us"][i] - rf["us"][i], rf["e_us"][i])
        shares["du%d" % i] = E.share(bw["dus"][i] - rb["dus"][i], rb["e_dus"][i])
        shares["dh%d" % i] = E.share(bw["dhs"][i] - rb["dhs"][i], rb["e_dhs"][i])
    for k in ("dwin", "dc", "dw0", "db0", "dz"):
        shares[k] = E.share(bw[k] - rb[k], rb["e_" + k])
    ofw, obw, free = E.output_end(w, inp["S"], E.LAYERS, inp["dwav"], dt=f4)
    qf, qb, qfree = ref["ofw"], ref["obw"], ref["free"]
    assert qfree["y1"].mean() <= E.MAX_FREE and qfree["s"].mean() <= E.MAX_FREE
    for k in ("y1", "wav"):
        shares[k] = E.share(ofw[k] - qf[k], qf["e_" + k])
    shares["dy1"] = E.share(obw["dy1"] - qb["dy1"], qb["e_dy1"], qfree["y1"])
    shares["ds"] = E.share(obw["ds"] - qb["ds"], qb["e_ds"], qfree["s"])
    for k in ("dW1", "db1", "dw3", "db3"):
        shares[k] = E.share(obw[k] - qb[k], qb["e_" + k])
    print(shape, A, ctx, Rc, "free %.2e" % qfree["y1"].mean(), {k: round(v, 4) for k, v in shares.items()})
    assert max(shares.values()) <= 1.0, shares
    assert min(shares[k] for k in ("cu", "wav", "dwin", "dW1")) > 0  # (float32 really differs: the comparison is not empty)


WHERE = {"across_edge": "cu", "stretch_off_by_one": "cu", "context_offset_dropped": "cu", "taps_reversed_bwd": "du", "dh_one_channel": "dh",
         "no_sigma_in_ds": "ds", "s_mask_dropped": "ds", "db3_missing": "db3"}


@pytest.mark.parametrize("mutant", (None,) + E.MUTANTS)
def test_mutants_leave_their_bound(mutant):
    """each in float64 on a case of the GPU tests: only the mutation separates it from the statement.  None: the statement itself is inside (at zero)."""
    ref = E.reference("hop6", 16, 2, 16)
    w, inp, frames, scales = ref["w"], ref["inp"], ref["frames"], ref["scales"]
    fw = E.input_forward(w, inp["c"], inp["z"], frames, scales, 2, mutant)
    bw = E.input_backward(w, inp["c"], inp["z"], ref["fw"], inp["dcu"], inp["dx0"], frames, scales, 2, mutant)
    _, obw, _ = E.output_end(w, inp["S"], E.LAYERS, inp["dwav"], mutant)
    rf, rb, qb = ref["fw"], ref["bw"], ref["obw"]
    shares = dict(cu=E.share(fw["cu"] - rf["cu"], rf["e_cu"]), du=max(E.share(a - b, e) for a, b, e in zip(bw["dus"], rb["dus"], rb["e_dus"])),
                  dh=max(E.share(a - b, e) for a, b, e in zip(bw["dhs"], rb["dhs"], rb["e_dhs"])), ds=E.share(obw["ds"] - qb["ds"], qb["e_ds"], ref["free"]["s"]),
                  db3=E.share(obw["db3"] - qb["db3"], qb["e_db3"]))
    if mutant is None:
        assert max(shares.values()) == 0.0
    else:
        assert shares[WHERE[mutant]] > 1.0, (mutant, shares)
        # nothing else moves, but for what is computed from the mutated array: the earlier stages' filter gradients read the later stages' du
        after = ("dh",) if mutant == "taps_reversed_bwd" else ()
        assert all(v == 0.0 for k, v in shares.items() if k != WHERE[mutant] and k not in after), (mutant, shares)


def test_refusals_name_the_argument(G):
    for scales in ([], [4] * 7, [1, 4], [4, 17], [4.0, 4]):
        with pytest.raises(ValueError, match=r"PWG generator: upsample_scales="):
            G.check_ends(scales, 2)
    for ctx in (-1, 9, 2.0):
        with pytest.raises(ValueError, match=r"PWG generator: aux_context_window="):
            G.check_ends([4, 4], ctx)
    for scales, ctx in (([2], 0), ([16] * 6, 8), ((4, 4, 4, 4), 2)):
        G.check_ends(scales, ctx)
    # a geometry the ends do not cover still constructs (its stack and the torch ends serve it) and is refused where the HIP ends are asked for
    gen = G.TrainableParallelWaveGANGenerator(layers=2, stacks=1, residual_channels=16, gate_channels=32, skip_channels=16, aux_channels=16,
                                              upsample_params={"upsample_scales": [32]})
    assert gen.hop == 32


def test_c_entries_validate_without_a_gpu(tmp_path):
    import __graft_entry__ as ge

    ge.build()
    from fcl_taco2_amd import _lib

    lib = _lib.load()
    in_fwd, in_bwd, out_fwd, out_bwd = entries = (lib.fcl_pwe_in_fwd, lib.fcl_pwe_in_bwd, lib.fcl_pwe_out_fwd, lib.fcl_pwe_out_bwd)
    for f in entries:
        assert f(None, None) == -1 and b"null" in lib.fcl_last_error()
    T = _lib.PweEnds
    single = [n for n, t in T._fields_ if t is C.c_void_p]
    assert len(single) == 33 and C.sizeof(T) == 8 + 4 * 6 + 4 * 6 + 8 + 8 * (33 + 18) + 8

    def ends(**kw):
        a = T()
        a.samples, a.frames, a.n_utt, a.residual, a.aux, a.ctx, a.n_scales, a.sigma = 100 * 256, 100, 3, 64, 80, 2, 4, 0.5
        for i in range(4):
            a.scales[i] = 4
        for n in single:
            setattr(a, n, 256)
        for n in ("h", "u", "dh"):
            for i in range(6):
                getattr(a, n)[i] = 256
        a.workspace_bytes = 1 << 40
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(a, k)[v[0]] = v[1]
            else:
                setattr(a, k, v)
        return a

    for f in entries:
        for bad in (dict(residual=60), dict(residual=80), dict(residual=8), dict(aux=72), dict(aux=144), dict(aux=0)):
            assert f(C.byref(ends(**bad)), None) == -2 and b"multiple of 16" in lib.fcl_last_error(), bad
        for bad in (dict(ctx=-1), dict(ctx=9)):
            assert f(C.byref(ends(**bad)), None) == -2 and b"aux_context_window" in lib.fcl_last_error(), bad
        for bad in (dict(n_scales=0), dict(n_scales=7)):
            assert f(C.byref(ends(**bad)), None) == -2 and b"upsample scales" in lib.fcl_last_error(), bad
        for bad in (dict(scales=(1, 1)), dict(scales=(3, 17))):
            assert f(C.byref(ends(**bad)), None) == -2 and b"upsample scale" in lib.fcl_last_error(), bad
        assert f(C.byref(ends(n_utt=0)), None) == -2 and f(C.byref(ends(n_utt=101)), None) == -2
        assert f(C.byref(ends(samples=100 * 256 + 1)), None) == -2 and b"frames x hop" in lib.fcl_last_error()
        assert f(C.byref(ends(samples=2 ** 31, frames=2 ** 23)), None) == -2
        for n in ("seg_lo", "seg_hi", "frame_off"):
            assert f(C.byref(ends(**{n: None})), None) == -1, n
    for n in ("c", "z", "w_in", "w0", "b0", "cu", "x0"):
        assert in_fwd(C.byref(ends(**{n: None})), None) == -1, n
    assert in_fwd(C.byref(ends(h=(3, None))), None) == -1 and in_fwd(C.byref(ends(u=(0, None))), None) == -1
    for n in ("dcu", "dx0", "c", "z", "w_in", "w0", "workspace"):
        assert in_bwd(C.byref(ends(**{n: None})), None) == -1, n
    for bad in (dict(dw0=None), dict(db0=None), dict(dh=(2, None)), dict(dw_in=None)):
        assert in_bwd(C.byref(ends(**bad)), None) == -1 and b"together" in lib.fcl_last_error(), bad
    assert in_bwd(C.byref(ends(u=(1, None))), None) == -1 and in_bwd(C.byref(ends(h=(1, None))), None) == -1
    assert in_bwd(C.byref(ends(workspace=260)), None) == -3
    need = lib.fcl_pwe_workspace_bytes(C.byref(ends()))
    n, Rc, A = 100 * 256, 64, 80
    assert need == 4 * (25 * (Rc + 1) * Rc + 2 * (n // 4) * A) and lib.fcl_pwe_workspace_bytes(None) == 0
    small = ends(samples=6, frames=1, n_utt=1, residual=16, aux=16, ctx=8, n_scales=2, scales=(0, 2))
    small.scales[1] = 3
    assert lib.fcl_pwe_workspace_bytes(C.byref(small)) == 4 * (17 * 16 * 16 + 2 * 2 * 16)  # (conv_in's gradient is the largest partial here)
    assert in_bwd(C.byref(ends(workspace_bytes=need - 4)), None) == -5 and b"workspace" in lib.fcl_last_error()
    for f in (out_fwd, out_bwd):
        for s in (0.0, -0.5, 1.5, float("nan")):
            assert f(C.byref(ends(sigma=s)), None) == -2 and b"sigma" in lib.fcl_last_error(), s
    for n in ("skips", "w1", "b1", "w3", "b3", "y1", "wav"):
        assert out_fwd(C.byref(ends(**{n: None})), None) == -1, n
    for n in ("skips", "w1", "y1"):
        assert out_fwd(C.byref(ends(**{n: 260})), None) == -3 and b"16-byte" in lib.fcl_last_error(), n
    for n in ("skips", "y1", "dwav", "w1t", "w3", "dy1", "ds", "workspace"):
        assert out_bwd(C.byref(ends(**{n: None})), None) == -1, n
    for n in ("db1", "dw3", "db3", "dw1"):
        assert out_bwd(C.byref(ends(**{n: None})), None) == -1 and b"together" in lib.fcl_last_error(), n
    for n in ("skips", "y1", "w1t", "dy1", "ds", "workspace"):
        assert out_bwd(C.byref(ends(**{n: 264})), None) == -3, n
    assert out_bwd(C.byref(ends(workspace_bytes=need - 4)), None) == -5
    # the ctypes mirror is laid out like the header's struct
    names = ("scales", "sigma", "seg_lo", "h", "u", "cu", "dh", "dw_in", "skips", "dwav", "workspace", "workspace_bytes")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fcl_hip.h"\nint main(void) { printf("%zu' + " %zu" * len(names) + '\\n", sizeof(fcl_pwe_t)'
                   + "".join(", offsetof(fcl_pwe_t, %s)" % n for n in names) + "); return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out == [C.sizeof(T)] + [getattr(T, n).offset for n in names]
