"""python -m fcl_taco2_amd.train_vocoder on a tiny synthetic corpus written here: 5 wavs of 0.4 - 0.9 s at 16 kHz (sums of a few sinusoids under a slow
envelope, 16-bit PCM) plus one too short for a window; mels from FeatureExtractor at n_fft 512, hop 64, 16 mels, normalised with their own statistics.
Generator: 4 layers in 2 stacks, 16 residual / skip and 32 gate channels, 16 aux channels, context 2, scales (4, 4, 4) -- but 32 / 64 / 32 in the one
case whose checkpoint the inference generator has to load, which takes multiples of 32; discriminator: 4 layers, 16 channels;
batch 3 x 1 280 samples; STFT resolutions (512, 512) / (50, 30) / (240, 120) -- 512 is the smallest n_fft the loss supports, so the
second resolution keeps the hop and window of the issue's (256, 30, 120) on a 512-point transform; the discriminator starts after step 2, 4 steps, every interval 2."""
import json
import wave

import numpy as np
import pytest
import torch

from test_gpu_features import DEV

pytestmark = pytest.mark.gpu
FS, HOP, MELS = 16000, 64, 16
G_PARAMS = dict(layers=4, stacks=2, residual_channels=16, gate_channels=32, skip_channels=16, aux_channels=16, aux_context_window=2,
                upsample_params={"upsample_scales": [4, 4, 4]})
G_PARAMS_32 = dict(G_PARAMS, residual_channels=32, gate_channels=64, skip_channels=32)
D_PARAMS = dict(layers=4, conv_channels=16)
RESOLUTIONS = [(512, 50, 240), (512, 30, 120)]
# Steps 2 and 3 of the same seed with the generator's ends in HIP and in torch: two correct float32 paths drift apart through RAdam's first steps, and
# the size of that cannot be derived.  Measured once on the MI355X: over steps 2 - 3 the worst relative difference of a loss term between
# the two legs is 1.41e-07 (the adversarial term of step 3, one unit in the last place of its float32 value; the six other terms are equal to the last
# bit).  The margin is 4 x the worst observed.
WORST_SEEN = 1.41e-07
MARGIN = 4 * WORST_SEEN
SECONDS = {"u0": 0.4, "u1": 0.9, "u2": 0.55, "u3": 0.7, "u4": 0.62, "short": 0.05}


@pytest.fixture(scope="module")
def TV():
    assert torch.cuda.is_available()
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import train_vocoder

    return train_vocoder


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    from fcl_taco2_amd import features as FX

    root = tmp_path_factory.mktemp("pwg_corpus")
    (root / "wavs").mkdir()
    (root / "feats" / "mels").mkdir(parents=True)
    rng, xs = np.random.RandomState(12), {}
    for u, secs in SECONDS.items():
        n = int(secs * FS)
        t = np.arange(n) / FS
        x = sum(a * np.sin(2 * np.pi * f * t + p) for a, f, p in zip(rng.uniform(0.1, 0.3, 4), rng.uniform(100, 3000, 4), rng.uniform(0, 6, 4)))
        x = x * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t + rng.uniform(0, 6)))
        pcm = np.clip(np.rint(x / np.abs(x).max() * 0.8 * 32767), -32768, 32767).astype("<i2")
        with wave.open(str(root / "wavs" / (u + ".wav")), "wb") as f:
            f.setnchannels(1), f.setsampwidth(2), f.setframerate(FS)
            f.writeframes(pcm.tobytes())
        xs[u] = pcm.astype(np.float32) / np.float32(32768.0)
    fx = FX.FeatureExtractor(FX.FeaturePlan(DEV, fs=FS, n_fft=512, hop=HOP, win_length=512, n_mels=MELS, fmin=80, fmax=7600))
    mels = {u: m.cpu().numpy() for u, (m, _) in zip(xs, fx.extract(list(xs.values())))}
    allm = np.concatenate(list(mels.values()))
    mean, std = allm.mean(0), allm.std(0)
    for u, m in mels.items():
        assert m.shape == (len(xs[u]) // HOP + 1, MELS)
        np.save(root / "feats" / "mels" / (u + ".npy"), ((m - mean) / std).astype(np.float32))
    (root / "train.txt").write_text("\n".join(["u0", "u1", "u2", "u3", "short"]) + "\n")
    (root / "valid.txt").write_text("u4\n")
    return root


def argv_of(corpus, outdir, *more):
    return ["--wav-dir", str(corpus / "wavs"), "--feature-root", str(corpus / "feats"), "--train-list", str(corpus / "train.txt"), "--valid-list",
            str(corpus / "valid.txt"), "--outdir", str(outdir), "--sampling-rate", str(FS), "--generator-params", json.dumps(G_PARAMS),
            "--discriminator-params", json.dumps(D_PARAMS), "--batch-size", "3", "--batch-max-steps", "1280", "--fft-sizes", "512,512", "--hop-sizes", "50,30",
            "--win-lengths", "240,120", "--discriminator-train-start-steps", "2", "--train-max-steps", "4", "--save-interval-steps", "2",
            "--eval-interval-steps", "2", "--log-interval-steps", "2", "--seed", "3", "--verbose", "0"] + list(more)


@pytest.fixture(scope="module")
def run4(TV, corpus, tmp_path_factory):
    out = tmp_path_factory.mktemp("run4")
    TV.main(argv_of(corpus, out))
    return out


def states(path):
    ck = torch.load(path, map_location="cpu", weights_only=True)
    flat = {}
    for net in ("generator", "discriminator"):
        flat.update({"model.%s.%s" % (net, k): v for k, v in ck["model"][net].items()})
        for i, st in ck["optimizer"][net]["state"].items():
            flat.update({"optimizer.%s.%s.%s" % (net, i, k): torch.as_tensor(v) for k, v in st.items()})
    return ck, flat


def test_four_steps_move_the_right_parameters_and_log_what_is_promised(TV, corpus, run4):
    ck2, _ = states(run4 / "checkpoint-2steps.pkl")
    ck4, _ = states(run4 / "checkpoint-4steps.pkl")
    assert ck2["steps"] == 2 and ck4["steps"] == 4 and ck4["epochs"] == 2  # (12 items over 4 utterances: the third epoch is running)
    first = TV.Trainer(TV.resolve(TV.build_parser().parse_args(argv_of(corpus, run4))), torch.device(DEV))  # the same seed: the initial weights
    g0, d0 = ({k: v.detach().cpu() for k, v in m.state_dict().items()} for m in (first.gen, first.disc))
    # two parameters cannot move: the last block's conv1x1_out feeds nothing, and first_conv.weight_v is one scalar per output channel under weight
    # norm, w = g v / |v|, whose derivative with respect to v is identically zero (only first_conv.weight_g and its bias train that layer)
    still = ("conv_layers.3.conv1x1_out.", "first_conv.weight_v")
    for k, v in ck4["model"]["generator"].items():
        assert torch.isfinite(v).all() and torch.equal(v, g0[k]) == k.startswith(still), k
    for k, v in ck2["model"]["discriminator"].items():
        assert torch.equal(v, d0[k]), k  # not before step 3
    for k, v in ck4["model"]["discriminator"].items():
        assert torch.isfinite(v).all() and not torch.equal(v, d0[k]), k
    lines = [json.loads(ln) for ln in (run4 / "train_log.jsonl").read_text().splitlines()]
    assert lines[0] == {"left_out": ["short"]}
    logs, evals = [r for r in lines if "ms_per_step" in r], [r for r in lines if "eval_windows" in r]
    assert [r["step"] for r in logs] == [2, 4] and [r["step"] for r in evals] == [2, 4]
    keys = {"step", "spectral_convergence_loss", "log_stft_magnitude_loss", "adversarial_loss", "real_loss", "fake_loss", "generator_lr", "discriminator_lr",
            "generator_grad_norm", "discriminator_grad_norm", "ms_per_step", "samples_per_second"}
    for r in logs:
        assert set(r) == keys and r["generator_lr"] == 1e-4 and r["discriminator_lr"] == 5e-5
    assert all(logs[0][k] is None for k in ("adversarial_loss", "real_loss", "fake_loss", "discriminator_grad_norm"))
    assert all(np.isfinite(v) for k, v in logs[0].items() if v is not None) and all(np.isfinite(v) for v in logs[1].values())
    assert set(evals[0]) == {"step", "eval_windows", "eval_spectral_convergence_loss", "eval_log_stft_magnitude_loss"} and evals[0]["eval_windows"] == 1
    assert "eval_adversarial_loss" in evals[1] and all(np.isfinite(v) for v in evals[1].values())


def test_the_decoders_load_the_checkpoint(TV, corpus, tmp_path):
    from fcl_taco2_amd import vocoder, vocoder_decode as VD
    from fcl_taco2_amd.kaldi_io import ArkScpWriter

    run4 = tmp_path / "run32"  # (32 residual channels: the smallest the inference generator loads)
    argv = argv_of(corpus, run4)
    argv[argv.index("--generator-params") + 1] = json.dumps(G_PARAMS_32)
    TV.main(argv)

    mel = np.load(corpus / "feats" / "mels" / "u4.npy")
    with ArkScpWriter(str(tmp_path / "feats")) as w:
        w["u4"] = mel
    samples, _ = VD.main(["--checkpoint", str(run4 / "checkpoint-4steps.pkl"), "--feats-scp", str(tmp_path / "feats.scp"), "--outdir", str(tmp_path / "wav"),
                          "--verbose", "0"])
    with wave.open(str(tmp_path / "wav" / "u4_gen.wav")) as f:
        assert (f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()) == (1, 2, FS, mel.shape[0] * HOP) and samples == mel.shape[0] * HOP
    ck = torch.load(run4 / "checkpoint-4steps.pkl", map_location="cpu", weights_only=True)
    cfg, _ = VD.generator_config(str(run4 / "checkpoint-4steps.pkl"))
    plan = vocoder.PWGPlan({k: v.numpy() for k, v in ck["model"]["generator"].items()}, DEV, cfg)
    assert plan.A == MELS


def test_resume_gives_the_bytes_of_the_uninterrupted_run(TV, corpus, run4, tmp_path):
    TV.main(argv_of(corpus, tmp_path, "--train-max-steps", "2"))
    TV.main(argv_of(corpus, tmp_path, "--resume", str(tmp_path / "checkpoint-2steps.pkl")))
    (_, a), (_, b) = states(run4 / "checkpoint-4steps.pkl"), states(tmp_path / "checkpoint-4steps.pkl")
    assert set(a) == set(b) and len([k for k in a if k.startswith("optimizer.discriminator")]) > 0
    for k in a:
        assert torch.equal(a[k], b[k]), k
    (_, a2), (_, b2) = states(run4 / "checkpoint-2steps.pkl"), states(tmp_path / "checkpoint-2steps.pkl")
    assert all(torch.equal(a2[k], b2[k]) for k in a2)
    with pytest.raises(ValueError, match="batch_size"):
        TV.main(argv_of(corpus, tmp_path, "--resume", str(tmp_path / "checkpoint-2steps.pkl"), "--batch-size", "2"))
    # --pretrain loads the models only: the step count starts over
    out = tmp_path / "pre"
    tr = TV.main(argv_of(corpus, out, "--pretrain", str(run4 / "checkpoint-4steps.pkl"), "--train-max-steps", "2"))
    assert tr.steps == 2 and (out / "checkpoint-2steps.pkl").exists()


def test_a_nan_in_a_mel_stops_the_run_naming_step_and_term(TV, corpus, tmp_path):
    import shutil

    bad = tmp_path / "feats" / "mels"
    shutil.copytree(corpus / "feats" / "mels", bad)
    m = np.load(bad / "u1.npy")
    m[:, 3] = np.nan
    np.save(bad / "u1.npy", m)
    argv = argv_of(corpus, tmp_path / "out")
    argv[argv.index("--feature-root") + 1] = str(tmp_path / "feats")
    with pytest.raises(FloatingPointError, match=r"step 1: (spectral_convergence_loss|log_stft_magnitude_loss|generator_grad_norm) is nan"):
        TV.main(argv)
    assert not list((tmp_path / "out").glob("checkpoint-*"))


def test_no_utterance_long_enough_is_refused_before_the_device(TV, corpus, tmp_path):
    (tmp_path / "only_short.txt").write_text("short\n")
    argv = argv_of(corpus, tmp_path / "out")
    argv[argv.index("--train-list") + 1] = str(tmp_path / "only_short.txt")
    with pytest.raises(ValueError, match="no utterance is long enough.*short"):
        TV.main(argv)
    assert not (tmp_path / "out").exists()


def test_no_discriminator_weight_gradient_in_the_generators_adversarial_backward(TV, corpus, tmp_path):
    """by the launch record: the discriminator runs forward and backward to its input, and none of its weight-gradient kernels is launched"""
    from test_gpu_pwg_generator import record

    tr = TV.Trainer(TV.resolve(TV.build_parser().parse_args(argv_of(corpus, tmp_path))), torch.device(DEV))
    z, c, wav = torch.randn(3, 1, 1280, device=DEV), torch.randn(3, 16, 24, device=DEV), 0.3 * torch.randn(3, 1, 1280, device=DEV)
    with record() as seen:
        _, terms = tr.losses(z, c, wav, True)
        assert all(p.requires_grad for p in tr.disc.parameters())  # released again before the backward pass
        tr.disc.zero_grad()
        sum(terms.values()).backward()
    assert "pwd_conv_kernel<fwd>" in seen and "pwd_conv_kernel<dx>" in seen and not [k for k in seen if k.startswith("pwd_dw")]
    assert all(p.grad is None for p in tr.disc.parameters()) and all(p.grad is not None for p in tr.gen.parameters())
    with record() as seen:  # (the control: the discriminator's own update does launch them)
        tr.disc(wav).square().mean().backward()
    assert [k for k in seen if k.startswith("pwd_dw")]


def test_three_steps_with_hip_ends_against_torch_ends(TV, corpus, tmp_path):
    """the same seed, 3 steps, --ends hip against --ends torch, every step's terms from the log (interval 1).  Step 1 (spectral convergence and log
    magnitude; no adversarial term yet) starts from the same weights: each leg within the bound of a float32 evaluation -- pwge_ref.generator's running
    bound of the waveform carried through the STFT loss by pwge_ref.stft_loss_bounds -- of the float64 statement, and the two within the sum.  That
    bound is printed: at 4 blocks and Kaiming weights the generator's running bound exceeds the waveform itself, so it admits far more than the two
    legs differ by; steps 2 - 3 are what pins them, within the measured margin."""
    import pwge_ref as E

    logs = {}
    for ends in ("hip", "torch"):
        out = tmp_path / ends
        argv = argv_of(corpus, out, "--ends", ends, "--train-max-steps", "3")
        argv[argv.index("--log-interval-steps") + 1] = "1"
        TV.main(argv)
        logs[ends] = [r for r in (json.loads(ln) for ln in (out / "train_log.jsonl").read_text().splitlines()) if "ms_per_step" in r]
        assert [r["step"] for r in logs[ends]] == [1, 2, 3]
    # step 1 in float64: the initial weights (the seed's), the batch and the noise of step 1
    cfg = TV.resolve(TV.build_parser().parse_args(argv_of(corpus, tmp_path)))
    tr = TV.Trainer(cfg, torch.device(DEV))
    tr.gen.remove_weight_norm()
    sd = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in tr.gen.state_dict().items()}
    gp = cfg["generator_params"]
    gcfg = dict({k: gp[k] for k in ("layers", "stacks", "residual_channels", "gate_channels", "skip_channels", "aux_channels", "aux_context_window",
                                    "kernel_size")}, upsample_scales=tuple(gp["upsample_params"]["upsample_scales"]))
    ids = [ln.split()[0] for ln in (corpus / "train.txt").read_text().splitlines()]
    lengths = [(u, np.load(corpus / "feats" / "mels" / (u + ".npy")).shape[0]) for u in ids]
    sampler = TV.Windows(lengths, 20, 2, HOP, 3, cfg["seed"])
    cs, ws = [], []
    for k, f0 in sampler.batch(1):
        u = sampler.utts[k][0]
        with wave.open(str(corpus / "wavs" / (u + ".wav"))) as f:
            pcm = np.frombuffer(f.readframes(f.getnframes()), dtype="<i2").astype(np.float32) / np.float32(32768.0)
        m, w = sampler.cut(np.load(corpus / "feats" / "mels" / (u + ".npy")), pcm, f0)
        cs.append(m)
        ws.append(w)
    z = sampler.noise(1)[:, 0]
    x, e, _, _ = E.generator(sd, gcfg, np.concatenate(cs), z.reshape(-1), np.ones(z.size, np.float32), [20, 20, 20])
    sc, mag, e_sc, e_mag = E.stft_loss_bounds(x.reshape(3, -1), e.reshape(3, -1), np.stack(ws).astype(np.float64), RESOLUTIONS)
    h, t = logs["hip"][0], logs["torch"][0]
    print("step 1: sc %.9g (hip %.9g, torch %.9g, bound %.3g), mag %.9g (hip %.9g, torch %.9g, bound %.3g); the waveform's bound is %.3g of its peak"
          % (sc, h["spectral_convergence_loss"], t["spectral_convergence_loss"], e_sc, mag, h["log_stft_magnitude_loss"], t["log_stft_magnitude_loss"],
             e_mag, e.max() / np.abs(x).max()))
    for name, ref, bound in (("spectral_convergence_loss", sc, e_sc), ("log_stft_magnitude_loss", mag, e_mag)):
        assert abs(h[name] - ref) <= bound and abs(t[name] - ref) <= bound and abs(h[name] - t[name]) <= 2 * bound, name
    worst = {}
    for a, b in zip(logs["hip"][1:], logs["torch"][1:]):
        for name in ("spectral_convergence_loss", "log_stft_magnitude_loss", "adversarial_loss", "real_loss", "fake_loss"):
            assert (a[name] is None) == (b[name] is None)
            if a[name] is not None:
                worst[(a["step"], name)] = abs(a[name] - b[name]) / max(abs(a[name]), abs(b[name]))
    print("steps 2 - 3, relative differences: %s; step 1: sc %.3g, mag %.3g" % (
        {k: float("%.3g" % v) for k, v in worst.items()}, abs(h["spectral_convergence_loss"] - t["spectral_convergence_loss"]) / sc,
        abs(h["log_stft_magnitude_loss"] - t["log_stft_magnitude_loss"]) / mag))
    assert (3, "adversarial_loss") in worst and max(worst.values()) <= MARGIN, worst
