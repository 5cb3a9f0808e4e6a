"""The hfe_* kernels of csrc/hifigan_end.hip and the module's output_end="hip" path against the float64 statement of tests/hfge_ref.py,
on the harness of test_gpu_hifigan_generator.py: every buffer a kernel writes sits between guard zones filled with a NaN bit pattern, which must survive,
and starts as NaN; every kernel test reads the library's launch record and fails if its kernels did not run.  The cases, their inputs and their bounds
are built and checked in hfge_ref.py / test_hifigan_end_cpu.py."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import hfge_ref as E
import hfgt_ref as R
import hifigan_ref as H
from test_gpu_features import DEV, Guarded, launched
from test_gpu_hifigan_generator import SMALL_ARGS, bw_names, module_inputs
from test_gpu_pwg_discriminator import share, split, t
from test_gpu_pwg_generator import record

pytestmark = pytest.mark.gpu
LENS, N = list(E.LENS), sum(E.LENS)
F64 = np.float64


@pytest.fixture(scope="module")
def G():
    assert torch.cuda.is_available()
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib, hifigan_generator

    _lib.load()
    return hifigan_generator


def call(entry, args):
    from fcl_taco2_amd import _lib, ops

    _lib.check(getattr(_lib.load(), entry)(C.byref(args), ops._stream()))


class Run(object):
    """the three launches of one packed batch on guarded buffers; the backward launches take `given` (the statement's waveform) as their wav"""

    def __init__(self, G, x, w, b, dwav, given, lens):
        from fcl_taco2_amd import _lib

        cout, c, k = w.shape
        n, maps, wp = len(x), G.Maps(lens, DEV), G.pack_end(t(w))
        A = functools.partial(G.end_args, maps, c, cout, k, E.OUT_SLOPE)
        xb, gb, db_, bias = Guarded(n, c).set(x), Guarded(n, cout).set(given), Guarded(n, cout).set(dwav), t(b)
        self.wav, self.dx, self.dw, self.db = Guarded(n, cout), Guarded(n, c), Guarded(k, cout, c), Guarded(cout)
        work = Guarded(_lib.load().fcl_hfe_workspace_bytes(n, c, cout, k) // 4)
        with launched(G.END_FWD):
            call("fcl_hfe_fwd", A(x=xb.t, w=wp, bias=bias, wav=self.wav.t))
        with launched(G.END_DX):
            call("fcl_hfe_dx", A(x=xb.t, w=wp, wav=gb.t, dwav=db_.t, dx=self.dx.t))
        with launched(*G.END_DW):
            call("fcl_hfe_dw", A(x=xb.t, wav=gb.t, dwav=db_.t, dw=self.dw.t, db=self.db.t, workspace=work.t))
        self.outputs = [self.wav, self.dx, self.dw, self.db]
        assert all(np.isfinite(o.np()).all() for o in self.outputs)
        assert all(o.intact() for o in self.outputs + [xb, gb, db_, work])


@functools.lru_cache(maxsize=None)
def case(c, cout, k):
    x, w, b, dwav = E.end_case(c, cout, k)
    return x, w, b, dwav, E.given_wav(x, w, b, LENS)


@pytest.mark.parametrize("c,cout,k", E.CELLS)
def test_each_launch_alone_vs_float64_and_twice_the_same_bits(G, c, cout, k):
    x, w, b, dwav, given = case(c, cout, k)
    run = Run(G, x, w, b, dwav, given, LENS)
    x64, w64, b64, d64, g64 = (np.asarray(v, F64) for v in (x, w, b, dwav, given))
    wav, e_wav = E.end_fwd(x64, w64, b64, LENS)
    dx, e_dx, unsure = E.end_dx(x64, w64, g64, d64, LENS)
    dW, db, e_dW, e_db = E.end_dw(x64, g64, d64, k, LENS)
    shares = dict(wav=share(run.wav.np() - wav, e_wav), dx=share(run.dx.np() - dx, e_dx), dw=share(run.dw.np().transpose(1, 2, 0) - dW, e_dW),
                  db=share(run.db.np() - db, e_db))
    print({n: round(v, 4) for n, v in shares.items()})
    assert unsure == 0.0 and max(shares.values()) <= 1.0
    again = Run(G, x, w, b, dwav, given, LENS)
    assert all(a.bits() == b_.bits() for a, b_ in zip(run.outputs, again.outputs))


@pytest.mark.parametrize("c,cout,k", E.CELLS)
def test_batch_is_its_utterances_alone_bit_for_bit(G, c, cout, k):
    x, w, b, dwav, given = case(c, cout, k)
    batch = Run(G, x, w, b, dwav, given, LENS)
    wavs, dxs = split(batch.wav.np(), LENS), split(batch.dx.np(), LENS)
    for i, (xx, dd, gg) in enumerate(zip(split(x, LENS), split(dwav, LENS), split(given, LENS))):
        alone = Run(G, xx, w, b, dd, gg, [LENS[i]])
        assert np.array_equal(alone.wav.np(), wavs[i]) and np.array_equal(alone.dx.np(), dxs[i]), i


def test_omission_rules_by_launch_counts(G):
    x, w, b, dwav, _ = case(32, 2, 5)
    plan = G.TrainingPlan(DEV, **SMALL_ARGS)
    maps = G.StageMaps(LENS, [], DEV)  # (only the last rate's tables are read: here the rows themselves)
    leaf = lambda a, grad: t(a).requires_grad_(grad)
    for gx, gw, gb in ((True, False, False), (False, True, False), (False, False, True), (True, True, True)):
        xin, ws, bs = leaf(x, gx), leaf(w, gw), leaf(b, gb)
        with record() as seen:
            wav = G.output_end(plan, maps, xin, ws, bs)
            torch.autograd.grad(wav, [v for v, g in ((xin, gx), (ws, gw), (bs, gb)) if g], grad_outputs=torch.ones_like(wav))
        assert seen[G.END_FWD]["launches"] == 1
        assert (G.END_DX in seen) == gx and (G.END_DW[0] in seen) == (gw or gb) and (G.END_DW[1] in seen) == (gw or gb), (gx, gw, gb)
    with record() as seen, torch.no_grad():
        G.output_end(plan, maps, xin.detach(), ws, bs)
    assert set(k_ for k_ in seen if k_.startswith("hfe_")) == {G.END_FWD}


def fold_tolerance(v, g, E_w, dLdw):
    """what an error E_w of the folded weight's gradient (the statement's dLdw) becomes in the gradients of weight_g and weight_v, w = v g / ||v|| over
    every dim but 0: dg = sum dw vhat, dv = s (dw - vhat sum dw vhat) with s = g / ||v||, vhat = v / ||v||; torch evaluates both in float32, 8 u of the
    terms' magnitudes"""
    red = tuple(range(1, v.ndim))
    nv = np.sqrt((v * v).sum(red, keepdims=True))
    vh, s = np.abs(v / nv), np.abs(g / nv)
    both = lambda e: ((e * vh).sum(red, keepdims=True), s * (e + vh * (e * vh).sum(red, keepdims=True)))
    (eg, ev), (mg, mv) = both(E_w), both(np.abs(dLdw))
    return eg + 8 * E.U * mg, ev + 8 * E.U * mv


@pytest.mark.parametrize("weight_norm", [False, True])
def test_module_hip_end_vs_torch_end_inside_the_sum_of_both_bounds(G, weight_norm):
    gen, sd, mel, dout, lens = module_inputs(G, weight_norm)
    plan, hop = gen.plan(), gen.hop
    names = [n for i in range(len(plan.scales)) for n in bw_names(R.SMALL, i)]
    own = {n: w.detach().cpu().numpy().astype(F64) for n, w in zip(names, gen.stage_parameters())}
    own.update({"input_conv.weight": gen.input_conv.folded().detach().cpu().numpy().astype(F64), "input_conv.bias": gen.input_conv.bias.detach().cpu().numpy().astype(F64)})
    oc = gen.output_conv.conv
    wo, bo = oc.folded().detach().cpu().numpy().astype(F64), oc.bias.detach().cpu().numpy().astype(F64)
    T = max(lens)
    padded = np.zeros((len(lens), 80, T), np.float32)
    for b, m in enumerate(split(mel, lens)):
        padded[b, :, : lens[b]] = m.T
    dpad = np.random.RandomState(11).standard_normal((len(lens), 1, T * hop)).astype(np.float32)
    dwav = np.concatenate([dpad[b, :, : n * hop].T for b, n in enumerate(lens)]).astype(F64)
    hip = E.module_statement(R, own, wo, bo, R.SMALL, mel.astype(F64), lens, dwav)
    tor = E.module_statement(R, own, wo, bo, R.SMALL, mel.astype(F64), lens, dwav, e_tanh=E.TORCH_E_TANH)
    assert hip["unsure"] <= R.MASK_CAP
    params = dict(gen.named_parameters())
    res = {}
    for end in ("hip", "torch"):
        with record() as seen:
            wav = gen(t(padded), lens, output_end=end)
            grads = torch.autograd.grad(wav, list(params.values()), grad_outputs=t(dpad))
        assert (G.END_FWD in seen) == (G.END_DX in seen) == (G.END_DW[0] in seen) == (end == "hip")
        res[end] = (wav.detach().cpu().numpy().astype(F64), {k: g.cpu().numpy().astype(F64) for k, g in zip(params, grads)})
    (wav_h, g_h), (wav_t, g_t) = res["hip"], res["torch"]
    assert wav_h.shape == wav_t.shape == (len(lens), 1, T * hop)
    off, worst = 0, {}
    for b, n in enumerate(lens):
        rows = slice(off, off + n * hop)
        assert share(wav_h[b, 0, : n * hop, None] - hip["wav"][rows], hip["e_wav"][rows]) <= 1.0, b  # the hip path inside its own bound
        worst["wav"] = max(worst.get("wav", 0.0), share((wav_h - wav_t)[b, 0, : n * hop, None], hip["e_wav"][rows] + tor["e_wav"][rows]))
        assert not wav_h[b, 0, n * hop :].any()  # padding rows are exactly zero
        off += n * hop
    tol = {k: hip["e_grads"][k] + tor["e_grads"][k] for k in hip["grads"]}
    for k in hip["grads"]:
        if not weight_norm or k.endswith("bias"):
            worst[k] = share(g_h[k] - g_t[k], tol[k])
            assert share(g_h[k] - hip["grads"][k], hip["e_grads"][k]) <= 1.0, k
        else:
            p = k[: -len("weight")]
            v, g = (params[p + n_].detach().cpu().numpy().astype(F64) for n_ in ("weight_v", "weight_g"))
            tg, tv = fold_tolerance(v, g, tol[k], hip["grads"][k])
            worst[p + "weight_g"], worst[p + "weight_v"] = share(g_h[p + "weight_g"] - g_t[p + "weight_g"], tg), share(g_h[p + "weight_v"] - g_t[p + "weight_v"], tv)
    print({k: round(v, 4) for k, v in worst.items()})
    assert set(worst) == set(params) | {"wav"} and max(worst.values()) <= 1.0


@pytest.mark.parametrize("weight_norm", [False, True])
def test_state_dict_loads_into_the_inference_plan(G, weight_norm):
    """the module's state_dict() in HiFiGANPlan: the module's own forward through the HIP end meets the inference path's bound of the float64 generator"""
    from fcl_taco2_amd import hifigan, vocoder

    gen, sd, mel, dout, lens = module_inputs(G, weight_norm)
    cfg = dict(R.SMALL, negative_slope=0.1)
    inf = hifigan.HiFiGANGenerator(hifigan.HiFiGANPlan(gen.state_dict(), DEV, H.plan_cfg(cfg)))
    wavs = inf.synthesize_packed(t(mel), lens)
    T, hop = max(lens), gen.hop
    padded = np.zeros((len(lens), 80, T), np.float32)
    for b, m in enumerate(split(mel, lens)):
        padded[b, :, : lens[b]] = m.T
    with torch.no_grad():
        own = gen(t(padded), lens, output_end="hip")
    folded = vocoder.fold_weight_norm(gen.state_dict())
    for b, (m, w) in enumerate(zip(split(mel, lens), wavs)):
        ref, mod = H.generator_f64(folded, m, cfg), H.generator_f64(folded, m, cfg, rnd=H.plane_round)
        peak, e_model = float(ref["wav"].abs().max()), float((mod["wav"] - ref["wav"]).abs().max())
        assert float((w.cpu().double().reshape(-1, 1) - ref["wav"]).abs().max()) <= H.bound(e_model, peak), b
        assert float((own[b, 0, : lens[b] * hop].cpu().double().reshape(-1, 1) - ref["wav"]).abs().max()) <= H.bound(e_model, peak), b
