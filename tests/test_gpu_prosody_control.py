"""-m gpu: prosody control (duration scale, pitch / energy affine) through the ctl kernels, the engine, the captured graph, the plug-in class
and the decode driver -- against the numpy rules of fcl_taco2_amd.prosody, the uncontrolled kernels and the CPU oracle."""
import argparse
import json

import numpy as np
import pytest
import torch

from helpers import max_abs, np_state_dict, torch_state_dict

pytestmark = pytest.mark.gpu

from fcl_taco2_amd import hparams as HP  # noqa: E402
from fcl_taco2_amd import prosody as P  # noqa: E402
from fcl_taco2_amd import synthetic as SYN  # noqa: E402
from oracle import fcl_oracle as O  # noqa: E402

DEV = "cuda:0"
ALPHAS = (0.1, 0.4, 0.5, 1.5, 2.0, 3.0)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from fcl_taco2_amd import _lib, ops as _ops

    _lib.load()
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _rigged_sd(hp):
    """Duration head weight 0, bias log 4: every phoneme predicts rint(4 - 1) = 3 (test_decode_driver_end_to_end's checkpoint)."""
    sd = torch_state_dict(hp, HP.teacher_hparams(), True)
    sd["duration_predictor.linear.weight"] = torch.zeros_like(sd["duration_predictor.linear.weight"])
    sd["duration_predictor.linear.bias"] = torch.full((1,), float(np.log(4.0)))
    return sd


def _plan(hp, sd):
    from fcl_taco2_amd.plan import SynthesisPlan

    return SynthesisPlan({k: (v.numpy() if torch.is_tensor(v) else v) for k, v in sd.items()}, hp, DEV)


def _student(sd):
    from fcl_taco2_amd.nets.knowledge_distillation.e2e_tts_tacotron2_sa_kd_student import Tacotron2_sa

    S = dict(embed_dim=256, eunits=256, econv_chans=256, dunits=256, postnet_chans=128, use_residual=False, use_masking=True, dropout_rate=0.0)
    com = argparse.Namespace(use_fe_condition=True, append_position=True, distill_output_knowledge=True, distill_encoder_knowledge=True,
                             distill_decoder_knowledge=True, distill_prosody_knowledge=True, is_train=True, share_proj=True)
    m = Tacotron2_sa(80, 80, argparse.Namespace(**S), com, argparse.Namespace(use_residual=False, use_masking=True))
    m.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()})
    return m.eval().to(DEV)


# ------------------------------------------------------------------------------------------------ 1. duration kernel
def test_duration_round_ctl_bit_exact(ops, golden):
    rng = np.random.RandomState(5)
    B, T = 4, 37
    n = B * T
    lin = np.concatenate([np.arange(0, 13, 0.5), rng.uniform(-2, 30, n - 26)]).astype(np.float32)  # integers, ties, negatives
    logits = rng.uniform(-1.0, 3.5, n).astype(np.float32)
    pad = (rng.rand(n) < 0.1).astype(np.uint8)
    alpha_u = np.array([0.5, 1.0, 1.5, 0.1], np.float32)
    alpha_r = rng.choice(np.array(ALPHAS + (1.0, 8.0, 0.37), np.float32), n)
    for x, linear in ((lin, True), (logits, False)):
        base = ops.duration_round(dev(x), linear, 1.0, dev(pad)).cpu().numpy()  # the uncontrolled integers
        nopad = ops.duration_round(dev(x), linear, 1.0, None).cpu().numpy()
        ctl_u = np.tile(np.array(P.IDENTITY, np.float32), (B, 1))
        ctl_u[:, 0] = alpha_u
        got = ops.duration_round_ctl(dev(x), dev(ctl_u), T, linear, 1.0, dev(pad)).cpu().numpy()
        want = np.where(pad == 1, 0, P.duration_rule(nopad, np.repeat(alpha_u, T)))
        assert np.array_equal(got, want)
        ctl_r = np.tile(np.array(P.IDENTITY, np.float32), (n, 1))
        ctl_r[:, 0] = alpha_r
        got = ops.duration_round_ctl(dev(x), dev(ctl_r), 1, linear, 1.0, dev(pad)).cpu().numpy()
        assert np.array_equal(got, np.where(pad == 1, 0, P.duration_rule(nopad, alpha_r)))
        assert np.array_equal(ops.duration_round_ctl(dev(x), None, 1, linear, 1.0, dev(pad)).cpu().numpy(), base)
    g = golden("g4_integer")
    for key, linear in (("lin", True), ("logits", False)):
        assert np.array_equal(ops.duration_round_ctl(dev(g[key]), None, 1, linear).cpu().numpy(), ops.duration_round(dev(g[key]), linear).cpu().numpy())
    assert np.array_equal(ops.duration_round_ctl(dev(g["lin"]), None, 1, True).cpu().numpy(), g["lin_round"])


# ------------------------------------------------------------------------------------------------ 2. embed kernel
def test_variance_embed_add_ctl(ops):
    rng = np.random.RandomState(1)
    hp = HP.student_hparams()
    sd = torch_state_dict(hp)
    lens = [9, 1, 30]
    T = 30
    M = len(lens) * T
    hs = rng.randn(M, hp.eunits).astype(np.float32)
    p, e = rng.randn(M).astype(np.float32), rng.randn(M).astype(np.float32)
    lo = np.repeat(np.arange(3) * T, T).astype(np.int32)
    hi = (lo + np.repeat(lens, T)).astype(np.int32)
    W = (dev(sd["pitch_embed.0.weight"].reshape(hp.eunits, -1).numpy()), dev(sd["pitch_embed.0.bias"].numpy()),
         dev(sd["energy_embed.0.weight"].reshape(hp.eunits, -1).numpy()), dev(sd["energy_embed.0.bias"].numpy()))
    args = (dev(hs), dev(p), dev(e)) + W + (dev(lo), dev(hi))
    out0, pe0, ee0 = ops.variance_embed_add(*args, want_embs=True)
    ident = np.tile(np.array(P.IDENTITY, np.float32), (M, 1))
    for ctl, div in ((ident, 1), (ident[:3], T), (None, 1)):
        out, pe, ee, po, eo = ops.variance_embed_add_ctl(*args, ctl=None if ctl is None else dev(ctl), ctl_row_div=div, want_embs=True)
        assert torch.equal(out, out0) and torch.equal(pe, pe0) and torch.equal(ee, ee0)
        assert torch.equal(po.cpu(), torch.from_numpy(p)) and torch.equal(eo.cpu(), torch.from_numpy(e))
    ctl = ident.copy()
    ctl[:, 1], ctl[:, 2] = rng.uniform(0.5, 2.0, M), rng.uniform(-1, 1, M)
    ctl[:, 3], ctl[:, 4] = rng.uniform(0.5, 2.0, M), rng.uniform(-1, 1, M)
    ctl[::4, 1:3] = (1.0, 0.0)  # some rows keep their pitch
    cu = ident[:3].copy()
    cu[:, 1:] = [[1.3, 0.2, 0.7, -0.1], [1.0, 0.0, 1.0, 0.0], [0.8, -0.5, 1.2, 0.3]]
    for c, div, crow in ((ctl, 1, ctl), (cu, T, np.repeat(cu, T, axis=0))):
        out, pe, ee, po, eo = ops.variance_embed_add_ctl(*args, ctl=dev(c), ctl_row_div=div, want_embs=True)
        p2, e2 = P.affine_rule(p, crow[:, 1], crow[:, 2]), P.affine_rule(e, crow[:, 3], crow[:, 4])
        assert max_abs(po.cpu(), p2) <= 1e-6 * max(1.0, float(np.abs(p2).max())) and max_abs(eo.cpu(), e2) <= 1e-6 * max(1.0, float(np.abs(e2).max()))
        _, pe_ref, ee_ref = ops.variance_embed_add(dev(hs), po, eo, *W, dev(lo), dev(hi), want_embs=True)
        assert torch.equal(pe, pe_ref) and torch.equal(ee, ee_ref)  # the stencil read exactly the values written to p_out / e_out
        for b, L in enumerate(lens):
            s = b * T
            rp = O.variance_embed(sd, "pitch", po.cpu()[s : s + L].reshape(1, L, 1))[0]
            re = O.variance_embed(sd, "energy", eo.cpu()[s : s + L].reshape(1, L, 1))[0]
            assert max_abs(pe[s : s + L].cpu(), rp) < 1e-5 and max_abs(ee[s : s + L].cpu(), re) < 1e-5
            assert max_abs(out[s : s + L].cpu(), torch.from_numpy(hs[s : s + L]) + rp + re) < 1e-5
    # rows with the identity pitch control keep the prediction bit for bit
    keep = (ctl[:, 1] == 1.0) & (ctl[:, 2] == 0.0)
    _, _, _, po, _ = ops.variance_embed_add_ctl(*args, ctl=dev(ctl), want_out=False)
    assert np.array_equal(po.cpu().numpy()[keep], p[keep])
    # scalars only: no embedding output, same controlled values
    _, _, _, po2, eo2 = ops.variance_embed_add_ctl(None, dev(p), dev(e), None, None, None, None, None, None, ctl=dev(ctl), want_out=False)
    assert torch.equal(po2, po)


# ------------------------------------------------------------------------------------------------ 3. duration scale end to end
def test_duration_scale_rigged_vs_oracle(ops):
    from fcl_taco2_amd import engine

    hp = HP.student_hparams(dropout_rate=0.0)
    sd = _rigged_sd(hp)
    plan = _plan(hp, sd)
    rng = np.random.RandomState(7)
    x = rng.randint(1, 80, size=23).astype(np.int64)
    T = len(x)
    for a in ALPHAS:
        d = int(P.duration_rule(np.array([3]), a)[0])
        mel = engine.synthesize(plan, [x], dropout_mode=ops.DROP_NONE, prosody=P.ProsodyControl(duration_scale=a))[0]
        assert mel.shape[0] == T * d, (a, mel.shape)
        with torch.no_grad():
            ref = O.inference(sd, hp, torch.from_numpy(x), dur=torch.full((T,), d, dtype=torch.int64))["after"]
        assert max_abs(mel.cpu(), ref) < 1e-3, a


# ------------------------------------------------------------------------------------------------ 4. predict -> override equivalence
def _mixed_controls(xs, rng):
    out = []
    for i, x in enumerate(xs):
        L = len(x)
        if i % 3 == 0:
            out.append(P.ProsodyControl(duration_scale=(0.6, 1.4, 1.0)[(i // 3) % 3], pitch_shift=0.3, energy_scale=1.2))
        elif i % 3 == 1:
            out.append(P.ProsodyControl(duration_scale=rng.uniform(0.5, 2.0, L), pitch_scale=rng.uniform(0.8, 1.2, L), pitch_shift=rng.uniform(-0.3, 0.3, L),
                                        energy_scale=rng.uniform(0.8, 1.2, L), energy_shift=rng.uniform(-0.2, 0.2, L)))
        else:
            out.append(None)
    return out


def test_predict_then_override_equals_controlled_pass(ops):
    hp = HP.student_hparams(dropout_rate=0.0)
    sd = SYN.positive_duration_head(np_state_dict(hp, HP.teacher_hparams(), True))
    model = _student(sd)
    xs, _ = SYN.batch_c2(hp.idim, batch=8, t_lo=20, t_hi=45, seed=21)
    ctls = _mixed_controls(xs, np.random.RandomState(4))
    pred = model.predict_prosody(xs, prosody=ctls)
    base = model.predict_prosody(xs)
    for b, c in enumerate(ctls):  # the predictions are the uncontrolled ones edited by the rules
        c = c or P.ProsodyControl()
        rows = c.rows(len(xs[b]))
        assert np.array_equal(pred["duration"][b], P.duration_rule(base["duration"][b], rows[:, 0]))
        assert max_abs(pred["pitch"][b], P.affine_rule(base["pitch"][b], rows[:, 1], rows[:, 2])) < 1e-6
    mel_c = model.inference_batch(xs, dropout_mode=ops.DROP_NONE, prosody=ctls)
    mel_o = model.inference_batch(xs, durs=pred["duration"], f0s=pred["pitch"], energies=pred["energy"], dropout_mode=ops.DROP_NONE)
    for a, b in zip(mel_c, mel_o):
        assert a.shape == b.shape and max_abs(a.cpu(), b.cpu()) <= 1e-6
    sdt = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
    for b in (0, 1):
        with torch.no_grad():
            ref = O.inference(sdt, hp, torch.from_numpy(xs[b]), dur=torch.from_numpy(pred["duration"][b]),
                              f0=torch.from_numpy(pred["pitch"][b]).reshape(-1, 1), energy=torch.from_numpy(pred["energy"][b]).reshape(-1, 1))["after"]
        assert max_abs(mel_c[b].cpu(), ref) < 1e-3
    with pytest.raises(ValueError):
        model.inference_batch(xs[:1], durs=pred["duration"][:1], prosody=P.ProsodyControl(duration_scale=2.0))
    with pytest.raises(ValueError):
        model.inference_batch(xs[:1], f0s=pred["pitch"][:1], energies=pred["energy"][:1], prosody=P.ProsodyControl(pitch_shift=0.1))


# ------------------------------------------------------------------------------------------------ 5-6. identity, BatchRunner
def test_identity_is_bit_identical_and_runner_replays_controls(ops):
    from fcl_taco2_amd import engine

    hp = HP.student_hparams(dropout_rate=0.0)
    plan = _plan(hp, SYN.positive_duration_head(np_state_dict(hp)))
    B, T_cap = 6, 48
    xs, _ = SYN.batch_c2(hp.idim, batch=B, t_lo=20, t_hi=T_cap, seed=9)
    plain = engine.synthesize(plan, xs, dropout_mode=ops.DROP_NONE)
    ident = engine.synthesize(plan, xs, dropout_mode=ops.DROP_NONE, prosody=P.ProsodyControl())
    assert all(torch.equal(a, b) for a, b in zip(plain, ident))
    sets = [P.ProsodyControl(duration_scale=0.5, pitch_shift=0.4),
            [P.ProsodyControl(duration_scale=1.5, energy_scale=0.7), None, P.ProsodyControl(pitch_scale=1.3)] * 2,
            [P.ProsodyControl(duration_scale=np.linspace(0.5, 2.0, len(x)), energy_shift=np.linspace(-0.3, 0.3, len(x))) for x in xs]]
    maps = []
    for s in [None] + sets:
        prep = engine.prepare(plan, xs, prosody=s)
        _, _, inter = engine.run(plan, prep, ops.DROP_NONE, return_intermediates=True)
        maps.append(inter["maps"])
    caps = engine.Caps.for_batches(maps, slack_steps=2)
    r0 = engine.BatchRunner(plan, B, T_cap, caps, forced=False, seed=5)
    r1 = engine.BatchRunner(plan, B, T_cap, caps, forced=False, seed=5, controls=True)
    assert r1._nbytes > r0._nbytes
    r0.load(xs)
    m0 = r0.replay()
    f0 = r0.frames()
    r1.load(xs)  # identity by default
    m1 = r1.replay()
    assert r1.frames() == f0 and torch.equal(m1[: sum(f0)], m0[: sum(f0)])
    r1.load(xs, prosody=P.ProsodyControl())
    m1 = r1.replay()
    assert r1.frames() == f0 and torch.equal(m1[: sum(f0)], m0[: sum(f0)])
    graph = r1.graph
    for s in sets:  # one capture, any control values
        r1.load(xs, prosody=s)
        mel = r1.replay()
        fr = r1.frames()
        ref = engine.synthesize(plan, xs, dropout_mode=ops.DROP_NONE, prosody=s)
        assert fr == [int(m.shape[0]) for m in ref]
        assert max_abs(mel[: sum(fr)], torch.cat(ref)) < 2e-5
    assert r1.graph is graph
    r1.load(xs, prosody=P.ProsodyControl(duration_scale=4.0))  # beyond the capacities: reported, never truncated
    r1.replay()
    with pytest.raises(ops._lib.FclError):
        r1.frames()
    with pytest.raises(ValueError):
        r0.load(xs, prosody=P.ProsodyControl(duration_scale=2.0))


# ------------------------------------------------------------------------------------------------ 7. no extra launches
def test_controlled_pass_makes_no_extra_launches(ops, monkeypatch):
    from fcl_taco2_amd import engine

    hp = HP.student_hparams(dropout_rate=0.0)
    plan = _plan(hp, SYN.positive_duration_head(np_state_dict(hp)))
    xs, _ = SYN.batch_c2(hp.idim, batch=4, t_lo=20, t_hi=40, seed=2)
    engine.synthesize(plan, xs, dropout_mode=ops.DROP_NONE)  # lazy setup out of the way
    calls = []
    real = ops.check

    def counting(rc):
        calls.append(1)
        return real(rc)

    monkeypatch.setattr(ops, "check", counting)
    engine.synthesize(plan, xs, dropout_mode=ops.DROP_NONE)
    n_plain = len(calls)
    del calls[:]
    engine.synthesize(plan, xs, dropout_mode=ops.DROP_NONE, prosody=P.ProsodyControl(duration_scale=1.3, pitch_shift=0.2, energy_scale=0.9))
    assert n_plain > 10 and len(calls) == n_plain


# ------------------------------------------------------------------------------------------------ 8-9. decode driver, plug-in route A
def _driver_files(tmp_path, golden, n=5):
    hp = HP.student_hparams(dropout_rate=0.0)
    sd = _rigged_sd(hp)
    torch.save({"model": sd, "optimizer": {}}, tmp_path / "snapshot.ep.1")
    args = dict(model_module="nets.knowledge_distillation.e2e_tts_tacotron2_sa_kd_student:Tacotron2_sa", embed_dim=256, eunits=256,
                econv_chans=256, dunits=256, postnet_chans=128, use_residual=False, use_masking=True, dropout_rate=0.0, share_proj=True)
    (tmp_path / "model.json").write_text(json.dumps([80, 80, args]))
    (tmp_path / "teacher.json").write_text(json.dumps([80, 80, dict(use_residual=False)]))
    g = golden("g2_student_c1")
    rng = np.random.RandomState(3)
    utts = {"u%02d" % i: {"output": [{"tokenid": " ".join(map(str, rng.randint(1, 80, size=rng.randint(5, 40))))}]} for i in range(n)}
    utts["g2"] = {"output": [{"tokenid": " ".join(map(str, g["x"].tolist()))}]}
    (tmp_path / "data.json").write_text(json.dumps({"utts": utts}))
    base = ["--model", str(tmp_path / "snapshot.ep.1"), "--model-conf", str(tmp_path / "model.json"), "--teacher-config", str(tmp_path / "teacher.json"),
            "--json", str(tmp_path / "data.json"), "--batch-size", "4", "--verbose", "0"]
    return hp, sd, g, {k: len(v["output"][0]["tokenid"].split()) for k, v in utts.items()}, base


def test_decode_driver_prosody_flags(ops, golden, tmp_path):
    from fcl_taco2_amd import decode as D
    from fcl_taco2_amd.kaldi_io import read_scp

    hp, sd, g, lens, base = _driver_files(tmp_path, golden)
    D.main(base + ["--out", str(tmp_path / "slow"), "--duration-scale", "2"])
    mels = read_scp(str(tmp_path / "slow.scp"))
    assert sorted(mels) == sorted(lens) and all(mels[k].shape == (6 * L, 80) for k, L in lens.items())
    stats = np.array([5.0, 0.3, 0.5, 1.7])
    np.save(tmp_path / "f0_en_stats.npy", stats)
    D.main(base + ["--out", str(tmp_path / "high"), "--semitones", "2", "--f0-en-stats", str(tmp_path / "f0_en_stats.npy")])
    mels = read_scp(str(tmp_path / "high.scp"))
    shift = np.float32(2.0 * np.log(2.0) / (12.0 * 0.3))
    x = torch.from_numpy(g["x"])
    with torch.no_grad():
        pred = O.inference(sd, hp, x)
        ref = O.inference(sd, hp, x, f0=pred["p_outs"].float() + float(shift), energy=pred["e_outs"].float())["after"]
    assert mels["g2"].shape == tuple(ref.shape) and max_abs(mels["g2"], ref) < 1e-3
    (tmp_path / "p.json").write_text(json.dumps({"u00": {"duration_scale": 0.5}, "u01": {"duration_scale": 3.0}, "g2": {"pitch_shift": 0.0}}))
    D.main(base + ["--out", str(tmp_path / "per"), "--prosody-json", str(tmp_path / "p.json")])
    mels = read_scp(str(tmp_path / "per.scp"))
    for k, L in lens.items():
        assert mels[k].shape[0] == {"u00": 2, "u01": 9}.get(k, 3) * L, k


def test_plugin_route_a_args_namespace(ops):
    hp = HP.student_hparams(dropout_rate=0.0)
    model = _student({k: v.numpy() for k, v in _rigged_sd(hp).items()})
    x = torch.from_numpy(np.random.RandomState(8).randint(1, 80, size=17).astype(np.int64)).to(DEV)
    assert model.inference(x, argparse.Namespace(duration_scale=2.0)).shape[0] == 6 * 17
    assert model.inference(x, argparse.Namespace(threshold=0.5)).shape[0] == 3 * 17
    assert model.inference(x, None, prosody={"duration_scale": 0.5}).shape[0] == 2 * 17
