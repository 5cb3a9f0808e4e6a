"""-m gpu: text -> waveform in one captured graph.  The capacity form of the vocoder (fcl_pwg_maps_build, the live-extent launches, fcl_pcm16_fwd;
vocoder.CapacitySynth) against the exact-size path (`synthesize_packed`, itself checked against oracle/pwg_oracle.py in test_gpu_vocoder.py),
engine.SpeechRunner against BatchRunner + synthesize_packed + the numpy PCM rule, and the one-process driver (fcl_taco2_amd/tts.py).
Closed-form weights (synthetic.py).

Bound of the waveform comparisons: the one the suite already uses for "same utterance, different call"
(test_gpu_vocoder.py::test_full_size_batch_equals_single_utterances): max_abs < 2e-4 x peak.  By construction (same tiles, same frame windows,
same absolute rows, same noise counter) capacity and exact form should be bit-identical; each test prints whether they were (observed on an
MI355X: bit-identical in every case, at the vocoder level and through SpeechRunner)."""
import json
import os
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

from test_speech_pipeline_cpu import EDGE, cases  # the same map cases (fixed + fuzzed) and PCM edge vector as the CPU statements of the rules

MAP_CASES = cases()


@pytest.fixture(scope="module")
def voc():
    assert torch.cuda.is_available()
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib, ops, vocoder

    _lib.load()
    if not ops.planes_enabled():
        pytest.skip("FCL_PRECISION=0 / FCL_PLANES=0: the vocoder needs the pre-split operand path")
    return vocoder


def weights(voc, cfg=None):
    from fcl_taco2_amd import synthetic as SYN

    return {k: SYN.closed_form_tensor("pwg." + k, tuple(s)) for k, s in voc.param_spec(cfg).items()}


@pytest.fixture(scope="module")
def gen(voc):
    return voc.ParallelWaveGANGenerator(voc.PWGPlan(weights(voc), DEV))


def build_maps(voc, lens, frames_cap, status=0, ctx=2, hop=256, utt_frame0=None):
    """fcl_pwg_maps_build into sentinel-filled buffers -> (dict of numpy arrays incl. live, status word afterwards)."""
    from fcl_taco2_amd import _lib, ops

    B = len(lens)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32) if utt_frame0 is None else np.asarray(utt_frame0, dtype=np.int32)
    pad_cap, m_cap = voc.capacity_sizes(B, frames_cap, ctx, hop)
    sizes = dict(pad_idx=pad_cap, lo=pad_cap, hi=pad_cap, keep=frames_cap, frame_utt=frames_cap, utt_off=B + 2, seg_lo=m_cap, seg_hi=m_cap, live=4)
    bufs = {k: torch.full((n,), -7, dtype=torch.int32, device=DEV) for k, n in sizes.items()}
    st = torch.tensor([status], dtype=torch.int32, device=DEV)
    f0 = torch.from_numpy(off).to(DEV)
    _lib.check(_lib.load().fcl_pwg_maps_build(f0.data_ptr(), st.data_ptr(), B, frames_cap, ctx, hop, *[bufs[k].data_ptr() for k in
                                              ("pad_idx", "lo", "hi", "keep", "frame_utt", "utt_off", "seg_lo", "seg_hi", "live")], ops._stream()))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in bufs.items()}, int(st.item()) & 0xFFFFFFFF


def assert_in_range(m, B, frames_cap, mel_rows, ctx=2, hop=256):
    pad_cap, m_cap = m["pad_idx"].shape[0], m["seg_lo"].shape[0]
    assert m["pad_idx"].min() >= 0 and m["pad_idx"].max() < max(mel_rows, 1)
    assert m["lo"].min() >= 0 and m["hi"].max() <= pad_cap and np.all(m["lo"] < m["hi"])
    assert m["keep"].min() >= 0 and m["keep"].max() < pad_cap
    assert m["frame_utt"].min() >= 0 and m["frame_utt"].max() <= B
    assert m["utt_off"].min() >= 0 and m["utt_off"].max() <= frames_cap and np.all(np.diff(m["utt_off"]) >= 0)
    assert m["seg_lo"].min() >= 0 and m["seg_hi"].max() <= m_cap and np.all(m["seg_lo"] < m["seg_hi"])


@pytest.mark.parametrize("case", range(len(MAP_CASES)))
def test_device_maps_equal_the_host_maps_and_the_rule(voc, gen, case):
    lens, cap = MAP_CASES[case]
    got, st = build_maps(voc, lens, cap)
    rule = voc.capacity_maps_rule(np.concatenate([[0], np.cumsum(lens)]), cap, 2, 256)
    assert st == 0 and rule["ok"]
    for k in ("pad_idx", "lo", "hi", "keep", "frame_utt", "utt_off", "seg_lo", "seg_hi", "live"):
        assert np.array_equal(got[k], rule[k]), k  # the whole capacity
    assert_in_range(got, len(lens), cap, cap)
    nz = [i for i, n in enumerate(lens) if n > 0]
    live = sum(lens)
    assert list(got["live"]) == [live, live * 256, live + 4 * len(nz), len(nz)]
    if nz:  # bit-exact against the generator's own host maps of the utterances that have frames
        mp = gen._maps([lens[i] for i in nz])
        torch.cuda.synchronize()
        lp = live + 4 * len(nz)
        for k, n in (("pad_idx", lp), ("lo", lp), ("hi", lp), ("keep", live), ("seg_lo", live * 256), ("seg_hi", live * 256)):
            assert np.array_equal(got[k][:n], mp[k].cpu().numpy()), k
        assert np.array_equal(got["frame_utt"][:live], np.asarray(nz, dtype=np.int32)[mp["frame_utt"].cpu().numpy()])  # numbered by slot
        assert np.array_equal(got["utt_off"][:-1], np.concatenate([[0], np.cumsum(lens)]))


@pytest.mark.parametrize("what", ["frames_over_cap", "incoming_status", "descending"])
def test_device_maps_overflow_and_incoming_status(voc, what):
    from fcl_taco2_amd import _lib, ops

    lens, cap, status, f0 = [5, 9, 3], 16, 0, None
    if what == "frames_over_cap":
        lens = [5, 9, 3]  # 17 > 16
    elif what == "incoming_status":
        lens, status = [5, 3], _lib.STATUS_FRAMES_CAP
    else:
        f0 = [0, 9, 4, 12]
    got, st = build_maps(voc, lens, cap, status=status, utt_frame0=f0)
    assert list(got["live"]) == [0, 0, 0, 0]
    assert st == (status | _lib.STATUS_VOCODER_CAP)
    assert "vocoder" in ops.status_message(st)
    assert_in_range(got, len(lens), cap, cap)
    assert np.all(got["frame_utt"] == len(lens)) and np.all(got["seg_lo"] == 0) and np.all(got["seg_hi"] == cap * 256)
    rule = voc.capacity_maps_rule(f0 if f0 is not None else np.concatenate([[0], np.cumsum(lens)]), cap, 2, 256, status=status)
    assert not rule["ok"]
    for k in ("pad_idx", "lo", "hi", "keep", "frame_utt", "seg_lo", "seg_hi", "live"):
        assert np.array_equal(got[k], rule[k]), k


def pcm16(x, live=None, status=None, cap=None):
    from fcl_taco2_amd import _lib, ops

    w = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)
    n = w.numel() if cap is None else cap
    out = torch.full((w.numel(),), 12345, dtype=torch.int16, device=DEV)
    st = torch.zeros(1, dtype=torch.int32, device=DEV) if status is None else status
    lv = None if live is None else torch.tensor([0, live, 0, 0], dtype=torch.int32, device=DEV)
    _lib.check(_lib.load().fcl_pcm16_fwd(w.data_ptr(), out.data_ptr(), n, None if lv is None else lv.data_ptr(), st.data_ptr(), ops._stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(st.item())


def test_pcm16_kernel_is_the_numpy_rule_bit_for_bit(voc, gen):
    from fcl_taco2_amd import _lib

    # a float32 times 32767 is exact in double; the only ties a float32 input can produce are odd multiples of 0.5 (+-0.5 in range -> +-16384)
    got, st = pcm16(EDGE)
    assert st == 0 and np.array_equal(got, voc.pcm16_rule(EDGE))
    rng = np.random.RandomState(3)
    x = (rng.standard_normal(100003) * 0.4).astype(np.float32)  # an odd count: the tail items
    got, st = pcm16(x)
    assert st == 0 and np.array_equal(got, voc.pcm16_rule(x))
    wav = gen.synthesize([rng.standard_normal((6, 80)).astype(np.float32)], seed=5)[0]
    real = (wav / wav.abs().max() * 1.2).cpu().numpy()  # a generator waveform scaled to clip here and there
    got, st = pcm16(real)
    assert st == 0 and np.array_equal(got, voc.pcm16_rule(real)) and got.max() == 32767
    # live word: nothing past it is written
    got, st = pcm16(x[:4096], live=1024)
    assert np.array_equal(got[:1024], voc.pcm16_rule(x[:1024])) and np.all(got[1024:] == 12345)
    # non-finite samples: 0 and the status bit
    y = x[:64].copy()
    y[5], y[17], y[40] = np.nan, np.inf, -np.inf
    got, st = pcm16(y)
    assert st == _lib.STATUS_PCM_NONFINITE and got[5] == 0 and got[17] == 0 and got[40] == 0 and np.array_equal(got, voc.pcm16_rule(y))


def _cap_vs_exact(voc, lens_slots, frames_cap, seed, explicit_noise, monkeypatch=None):
    """Capacity form against synthesize_packed on the same packed rows.  lens_slots may hold zeros (unused slots).  Returns (bit_identical, worst rel)."""
    from fcl_taco2_amd import _lib

    g = voc.ParallelWaveGANGenerator(voc.PWGPlan(weights(voc), DEV))
    rng = np.random.RandomState(seed)
    lens = [n for n in lens_slots if n > 0]
    total, hop = sum(lens), g.plan.hop
    mel = rng.standard_normal((total, 80)).astype(np.float32)
    mel_cap = torch.full((frames_cap + 13, 80), float("nan"), device=DEV)  # the rows past the total hold NaN
    mel_cap[:total] = torch.from_numpy(mel).to(DEV)
    noise = [rng.standard_normal(n * hop).astype(np.float32) for n in lens] if explicit_noise else None
    want = g.synthesize_packed(torch.from_numpy(mel).to(DEV), lens, noise=noise, seed=seed)
    cs = voc.CapacitySynth(g, len(lens_slots), frames_cap, seed=seed)
    M, live = cs.M, total * hop
    SENT, PNAN = 1.0e30, 0x7FC0  # plane sentinel: a bf16 NaN in both planes -- rows past the live edge must be unread, not multiplied by zero
    cs.skips.fill_(SENT); cs.wav.fill_(SENT); cs.xp.fill_(PNAN); cs.gp.fill_(PNAN); cs.pcm.fill_(12345)
    if explicit_noise:
        cs.z.fill_(float("nan"))
        cs.z[:live] = torch.from_numpy(np.concatenate(noise)).to(DEV)
    f0 = torch.from_numpy(np.concatenate([[0], np.cumsum(lens_slots)]).astype(np.int32)).to(DEV)
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    cs.run(mel_cap, f0, st, draw_noise=not explicit_noise)
    torch.cuda.synchronize()
    assert int(st.item()) == 0 and list(cs.live.cpu().numpy()[:2]) == [total, live]
    wav = cs.wav.cpu().numpy()
    assert np.all(np.isfinite(wav[:live]))
    ident, worst, s = True, 0.0, 0
    for i, n in enumerate(lens):  # every live sample of every utterance
        w = want[i].cpu().numpy()
        c = wav[s : s + n * hop]
        s += n * hop
        peak = float(np.abs(w).max())
        err = float(np.abs(c - w).max())
        ident = ident and np.array_equal(c, w)
        worst = max(worst, err / peak)
        assert peak > 0 and err < 2e-4 * peak, (i, err, peak)
    # work follows the live extent: nothing at or past the last live tile was touched
    edge = 128 * ((live + 127) // 128)
    assert bool((cs.wav[edge:] == SENT).all()) and bool((cs.skips[edge:] == SENT).all())
    assert bool((cs.xp[:, edge:] == PNAN).all()) and bool((cs.gp[:, edge:] == PNAN).all())
    assert bool((cs.pcm[live:] == 12345).all())
    assert np.array_equal(cs.pcm[:live].cpu().numpy(), voc.pcm16_rule(wav[:live]))
    print("capacity vs exact: lens %r cap %d explicit_noise %s -> bit-identical %s, worst rel %.3g" % (lens_slots, frames_cap, explicit_noise, ident, worst))
    return ident, worst


@pytest.mark.parametrize("explicit_noise", [False, True])
@pytest.mark.parametrize("lens_slots,frames_cap", [([5, 1, 3], 9), ([37, 1, 12, 0, 0], 96), ([3, 70, 33, 2], 300)])
def test_capacity_vocoder_equals_the_exact_one(voc, lens_slots, frames_cap, explicit_noise):
    _cap_vs_exact(voc, lens_slots, frames_cap, 4, explicit_noise)


@pytest.mark.parametrize("lens_slots,frames_cap", [([5, 1, 3], 9), ([37, 1, 12, 0, 0], 96)])
def test_capacity_vocoder_from_upsampled_planes(voc, lens_slots, frames_cap, monkeypatch):
    monkeypatch.setenv("FCL_PWG_AUX_FRAME_RATE", "0")
    _cap_vs_exact(voc, lens_slots, frames_cap, 6, False)
    _cap_vs_exact(voc, lens_slots, frames_cap, 6, True)


def test_capacity_vocoder_refuses_other_geometries(voc):
    from fcl_taco2_amd import _lib

    cfg = dict(layers=4, stacks=2, residual_channels=32, gate_channels=64, skip_channels=32, aux_channels=20, upsample_scales=(2, 3))
    g = voc.ParallelWaveGANGenerator(voc.PWGPlan(weights(voc, cfg), DEV, cfg))
    with pytest.raises(_lib.FclError, match="one-launch block"):
        voc.CapacitySynth(g, 4, 32)


# ------------------------------------------------------------------------------------------------ SpeechRunner
def _student_plan(rigged=False):
    from fcl_taco2_amd import hparams as HP, synthetic as SYN
    from fcl_taco2_amd.plan import SynthesisPlan

    hp = HP.student_hparams(dropout_rate=0.0)
    sd = SYN.positive_duration_head(SYN.closed_form_state_dict(HP.param_spec(hp)))
    return hp, SynthesisPlan(sd, hp, DEV)


def _check_batch(voc, gen, r, xs, want_frames=None):
    """load / replay / waveforms of one batch against BatchRunner's own mel + the exact-size vocoder + the numpy PCM rule."""
    r.load(xs) if want_frames is None else r.load(xs, prosody=want_frames[0])
    r.replay()
    pcm = r.waveforms()
    frames = r.frames()
    total = sum(frames)
    assert len(pcm) == len(xs) and [p.shape[0] for p in pcm] == [r.hop * f for f in frames] and all(p.dtype == np.int16 for p in pcm)
    assert min(frames) >= 1
    want = gen.synthesize_packed(r.mel[:total].clone(), frames, seed=r.noise_seed())
    torch.cuda.synchronize()
    s, ident = 0, True
    for i, w in enumerate(want):
        w = w.cpu().numpy()
        c = r.synth.wav[s : s + w.shape[0]].cpu().numpy()
        s += w.shape[0]
        peak = float(np.abs(w).max())
        assert peak > 0 and float(np.abs(c - w).max()) < 2e-4 * peak, i
        ident = ident and np.array_equal(c, w)
        ref = voc.pcm16_rule(w)
        assert np.abs(pcm[i].astype(np.int32) - ref.astype(np.int32)).max() <= 1
        if np.array_equal(c, w):
            assert np.array_equal(pcm[i], ref), i
    print("SpeechRunner batch of %d: %d frames, float waveform bit-identical to the exact path: %s" % (len(xs), total, ident))
    assert ident  # the capacity form was bit-identical in every vocoder-level comparison above; it must be here as well
    return frames, pcm


def test_speech_runner_one_graph_text_to_pcm(voc, gen):
    from fcl_taco2_amd import _lib, engine, ops, prosody as P, synthetic as SYN

    hp, plan = _student_plan()
    B, T_cap = 12, 48
    xs, _ = SYN.batch_c2(hp.idim, batch=B, t_lo=10, t_hi=T_cap, seed=9)
    xs2, _ = SYN.batch_c2(hp.idim, batch=7, t_lo=5, t_hi=40, seed=21)
    slow = P.ProsodyControl(duration_scale=1.5)
    maps = []
    for b_, s_ in ((xs, None), (xs2, None), (xs, slow)):
        _, _, inter = engine.run(plan, engine.prepare(plan, b_, prosody=s_), ops.DROP_NONE, return_intermediates=True)
        maps.append(inter["maps"])
    caps = engine.Caps.for_batches(maps[:2], slack_steps=2)
    r = engine.SpeechRunner(plan, gen, B, T_cap, caps, seed=5)
    assert r.forced is False and r.synth.frames_cap == caps.frames
    graph = r.graph
    frames1, pcm1 = _check_batch(voc, gen, r, xs)
    assert frames1 == list(maps[0].utt_frames)
    for _ in range(2):  # replays of one batch draw fresh noise (and fresh prenet masks)
        r.replay()
    again = r.waveforms()
    assert not np.array_equal(again[0], pcm1[0])
    frames2, _ = _check_batch(voc, gen, r, xs2)  # another batch, fewer utterances, through the SAME graph
    assert frames2 == list(maps[1].utt_frames) and r.graph is graph
    frames1b, _ = _check_batch(voc, gen, r, xs)
    assert frames1b == frames1
    torch.cuda.synchronize()
    mem = torch.cuda.memory_allocated()  # (taken here: the reference side of _check_batch caches its host-built maps in `gen`)
    for b_ in (xs2, xs, xs2):
        r.load(b_)
        r.replay()
        out = r.waveforms()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == mem and len(out) == len(xs2)  # nothing is allocated per batch
    # the vocoder's own capacity: exceeded while the synthesis capacities hold -> reported, nothing truncated
    small = engine.SpeechRunner(plan, gen, B, T_cap, caps, voc_frames_cap=sum(frames1) - 1, seed=5)
    small.load(xs)
    small.replay()
    with pytest.raises(_lib.FclError, match="vocoder capacity"):
        small.waveforms()
    small.load(xs2)  # a batch that fits runs through the same graph afterwards
    small.replay()
    assert [p.shape[0] for p in small.waveforms()] == [256 * f for f in frames2]
    del small
    # prosody controls: the sample counts follow the controlled frame counts
    caps_c = engine.Caps.for_batches(maps, slack_steps=2)
    rc = engine.SpeechRunner(plan, gen, B, T_cap, caps_c, seed=5, controls=True)
    frames_c, _ = _check_batch(voc, gen, rc, xs, want_frames=(slow,))
    assert frames_c == list(maps[2].utt_frames) and sum(frames_c) > sum(frames1)


def test_replay_has_no_host_round_trip():
    """Review aid kept as a test: SpeechRunner adds no replay() of its own, and BatchRunner.replay, both CapacitySynth.run and every shared function
    they enqueue through hold no synchronising call and no allocation (the chain builders allocate for the exact form: __init__ and
    synthesize_packed call them, run does not)."""
    import inspect

    from fcl_taco2_amd import engine, hifigan, vocoder

    assert engine.SpeechRunner.replay is engine.BatchRunner.replay
    for fn in (engine.BatchRunner.replay, vocoder.CapacitySynth.run, vocoder.CapacitySynth._cascade, vocoder.check_run_args, vocoder.cascade,
               vocoder.aux_term, hifigan.CapacitySynth.run, hifigan.enqueue_chain, engine.SpeechRunner._vocoder_tail):
        src = inspect.getsource(fn)
        for word in (".item()", ".cpu()", "synchronize", "torch.empty", "torch.zeros", ".to("):
            assert word not in src, (fn.__name__, word)


# ------------------------------------------------------------------------------------------------ driver
def _driver_files(voc, tmp_path, n=11):
    from fcl_taco2_amd import hparams as HP, synthetic as SYN

    hp = HP.student_hparams(dropout_rate=0.0)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in SYN.closed_form_state_dict(HP.param_spec(hp, HP.teacher_hparams(), True)).items()}
    sd["duration_predictor.linear.weight"] = torch.zeros_like(sd["duration_predictor.linear.weight"])
    sd["duration_predictor.linear.bias"] = torch.full((1,), float(np.log(4.0)))  # every phoneme predicts 3 frames
    torch.save({"model": sd, "optimizer": {}}, tmp_path / "snapshot.ep.1")
    args = dict(model_module="nets.knowledge_distillation.e2e_tts_tacotron2_sa_kd_student:Tacotron2_sa", embed_dim=256, eunits=256,
                econv_chans=256, dunits=256, postnet_chans=128, use_residual=False, use_masking=True, dropout_rate=0.0, share_proj=True)
    (tmp_path / "model.json").write_text(json.dumps([80, 80, args]))
    (tmp_path / "teacher.json").write_text(json.dumps([80, 80, dict(use_residual=False)]))
    rng = np.random.RandomState(3)
    utts = {"u%02d" % i: {"output": [{"tokenid": " ".join(map(str, rng.randint(1, 80, size=rng.randint(5, 40))))}]} for i in range(n)}
    (tmp_path / "data.json").write_text(json.dumps({"utts": utts}))
    vsd = weights(voc)
    torch.save({"model": {"generator": {k: torch.from_numpy(v) for k, v in vsd.items()}}}, tmp_path / "PWG.pkl")
    (tmp_path / "config.yml").write_text("sampling_rate: 24000\n")
    base = ["--model", str(tmp_path / "snapshot.ep.1"), "--model-conf", str(tmp_path / "model.json"), "--teacher-config", str(tmp_path / "teacher.json"),
            "--json", str(tmp_path / "data.json"), "--vocoder-checkpoint", str(tmp_path / "PWG.pkl"), "--batch-size", "3", "--verbose", "0", "--seed", "11"]
    return {k: len(v["output"][0]["tokenid"].split()) for k, v in utts.items()}, base


def _read_wav(path):
    with wave.open(str(path)) as f:
        return (f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()), np.frombuffer(f.readframes(f.getnframes()), dtype="<i2")


def test_tts_driver_writes_wavs_from_a_manifest(voc, gen, tmp_path):
    from fcl_taco2_amd import tts as TTS
    from fcl_taco2_amd.kaldi_io import read_scp

    lens, base = _driver_files(voc, tmp_path)
    res = TTS.main(base + ["--outdir", str(tmp_path / "wav"), "--feats-out", str(tmp_path / "feats")])
    n_batches = (len(lens) + 2) // 3
    assert res["graph_batches"] + res["eager_batches"] + res["redone_batches"] == n_batches == len(res["batches"])
    assert res["eager_batches"] >= 1 and res["graph_batches"] >= 1 and res["utterances"] == len(lens)
    assert res["samples"] == 256 * 3 * sum(lens.values()) and res["rtf"] > 0
    mels = read_scp(str(tmp_path / "feats.scp"))
    assert sorted(mels) == sorted(lens)
    for k, L in lens.items():
        hdr, pcm = _read_wav(tmp_path / "wav" / (k + "_gen.wav"))
        assert hdr == (1, 2, 24000, 256 * 3 * L) and mels[k].shape == (3 * L, 80) and np.abs(pcm).max() > 0
    # the ark holds exactly the mels the waveforms were made from: every batch redone from the ark by the exact-size vocoder gives the wav's bytes
    for route, ids, nseed in res["batches"]:
        rows = torch.from_numpy(np.concatenate([mels[k] for k in ids])).to(DEV)
        want = gen.synthesize_packed(rows, [mels[k].shape[0] for k in ids], seed=nseed)
        for k, w in zip(ids, want):
            assert np.array_equal(_read_wav(tmp_path / "wav" / (k + "_gen.wav"))[1], voc.pcm16_rule(w.cpu().numpy())), (route, k)
    # same seed, same bytes
    res2 = TTS.main(base + ["--outdir", str(tmp_path / "wav2")])
    assert res2["samples"] == res["samples"]
    for k in lens:
        assert (tmp_path / "wav" / (k + "_gen.wav")).read_bytes() == (tmp_path / "wav2" / (k + "_gen.wav")).read_bytes(), k
    # speaking rate from the shared prosody flags; and the plug-in entry for callers that hold a model
    res3 = TTS.main(base + ["--outdir", str(tmp_path / "slow"), "--duration-scale", "2"])
    assert res3["samples"] == 256 * 6 * sum(lens.values())


def test_model_synthesize_speech(voc, gen):
    from fcl_taco2_amd import hparams as HP, synthetic as SYN
    from fcl_taco2_amd.nets.knowledge_distillation.e2e_tts_tacotron2_sa_kd_student import Tacotron2_sa
    import argparse

    hp = HP.student_hparams(dropout_rate=0.0)
    sd = SYN.positive_duration_head(SYN.closed_form_state_dict(HP.param_spec(hp, HP.teacher_hparams(), True)))
    S = dict(embed_dim=256, eunits=256, econv_chans=256, dunits=256, postnet_chans=128, use_residual=False, use_masking=True, dropout_rate=0.0)
    com = argparse.Namespace(use_fe_condition=True, append_position=True, distill_output_knowledge=True, distill_encoder_knowledge=True,
                             distill_decoder_knowledge=True, distill_prosody_knowledge=True, is_train=True, share_proj=True)
    m = Tacotron2_sa(80, 80, argparse.Namespace(**S), com, argparse.Namespace(use_residual=False, use_masking=True))
    m.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()})
    m = m.eval().to(DEV)
    xs, _ = SYN.batch_c2(hp.idim, batch=3, t_lo=6, t_hi=20, seed=4)
    xs = [torch.from_numpy(x).to(DEV) for x in xs]
    pcm = m.synthesize_speech(xs, gen, seed=7)
    mels = m.inference_batch(xs, seed=7)
    want = gen.synthesize(mels, seed=7)
    assert len(pcm) == 3
    for p, w, mel in zip(pcm, want, mels):
        assert p.dtype == np.int16 and p.shape[0] == 256 * mel.shape[0] and np.array_equal(p, voc.pcm16_rule(w.cpu().numpy()))


def test_tts_driver_redoes_a_batch_that_overflows_its_capacities(voc, gen, tmp_path):
    """Every utterance but the three longest (the calibration batch) speaks four times slower: the estimated capacities of the later batches do not
    hold, the device reports it, the batch is redone through the two-step route, its bucket grows and the next batch of that bucket fits again."""
    from fcl_taco2_amd import tts as TTS

    lens, base = _driver_files(voc, tmp_path, n=16)
    order = sorted(lens, key=lambda k: -lens[k])
    (tmp_path / "p.json").write_text(json.dumps({k: {"duration_scale": 4.0} for k in order[3:]}))
    from fcl_taco2_amd.kaldi_io import read_scp

    res = TTS.main(base + ["--outdir", str(tmp_path / "wav"), "--prosody-json", str(tmp_path / "p.json"), "--max-buckets", "1",
                           "--feats-out", str(tmp_path / "feats")])
    assert res["redone_batches"] >= 2 and res["eager_batches"] == 1  # consecutive batches of one runner overflow: each is judged by its own status word
    mels = read_scp(str(tmp_path / "feats.scp"))
    for route, ids, nseed in res["batches"]:  # no batch's files hold another batch's samples: every wav is its own ark mels through the vocoder
        want = gen.synthesize_packed(torch.from_numpy(np.concatenate([mels[k] for k in ids])).to(DEV), [mels[k].shape[0] for k in ids], seed=nseed)
        for k, w in zip(ids, want):
            assert np.array_equal(_read_wav(tmp_path / "wav" / (k + "_gen.wav"))[1], voc.pcm16_rule(w.cpu().numpy())), (route, k)
    assert res["graph_batches"] + res["eager_batches"] + res["redone_batches"] == 6
    for k, L in lens.items():
        hdr, pcm = _read_wav(tmp_path / "wav" / (k + "_gen.wav"))
        assert hdr == (1, 2, 24000, 256 * 3 * L * (1 if k in order[:3] else 4)), k
        assert np.abs(pcm).max() > 0
    print("driver with overflowing batches:", {k: res[k] for k in ("graph_batches", "eager_batches", "redone_batches")})
