"""python -m fcl_taco2_amd.train_vocoder --generator-type HiFiGANGenerator on test_gpu_train_vocoder.py's tiny synthetic corpus (16 kHz, hop 64, 16 mels),
each case the twin of the Parallel WaveGAN one there.  Generator: 16 mels in, scales (4, 4, 4) with kernels (8, 8, 8), blocks (3, 7) x ((1, 3), (1, 5)) at
256 channels -- the issue names 128, which hifigan.config refuses for three stages (the inference generator takes multiples of 32 x 2^stages), so the
smallest width both generators take is used; discriminator: 2 scales of the narrowest shape (64 channels, 4 groups, kernels (5, 3, 3, 3), one
downsampling by 2) and periods (2, 3) at 16 channels, scales (3, 3, 1); mel loss at n_fft 512, hop 64, 16 mels; batch 3 x 1 280 samples; the
discriminator starts after step 2, 4 steps, every interval 2."""
import json
import wave

import numpy as np
import pytest
import torch

from test_gpu_features import DEV
from test_gpu_train_vocoder import FS, HOP, MELS, corpus, states  # noqa: F401  (corpus: the fixture, rebuilt for this module)

pytestmark = pytest.mark.gpu
G_PARAMS = dict(in_channels=16, channels=256, upsample_scales=[4, 4, 4], upsample_kernel_sizes=[8, 8, 8], resblock_kernel_sizes=[3, 7],
                resblock_dilations=[[1, 3], [1, 5]])
D_PARAMS = dict(scales=2, scale_discriminator_params=dict(channels=64, max_downsample_channels=64, max_groups=4, kernel_sizes=[5, 3, 3, 3], downsample_scales=[2]),
                periods=[2, 3], period_discriminator_params=dict(channels=16, downsample_scales=[3, 3, 1]))
MEL = dict(fs=FS, fft_size=512, hop_size=HOP, num_mels=MELS)
TERMS = ("mel_loss", "adversarial_loss", "feature_matching_loss", "real_loss", "fake_loss")
# Steps 1 - 3 of the same seed with the generator's output end in HIP and in torch: two correct float32 paths whose waveforms differ in the last bits, and
# drift apart through Adam's first steps; the size of that cannot be derived.  Measured once on the MI355X, against the torch-end leg:
# over steps 1 - 3 the worst relative difference of a loss term is 2.06e-07 (the discriminator's fake loss of step 3, two units in the last place of
# its float32 value; the mel term of step 2 differs by 9.6e-08, the five other logged terms are equal to the last bit).  The margin is 4 x the worst
# observed.
WORST_SEEN = 2.06e-07
MARGIN = 4 * WORST_SEEN


@pytest.fixture(scope="module")
def TV():
    assert torch.cuda.is_available()
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import train_vocoder

    return train_vocoder


def argv_of(corpus, outdir, *more):  # noqa: F811
    return ["--generator-type", "HiFiGANGenerator", "--wav-dir", str(corpus / "wavs"), "--feature-root", str(corpus / "feats"), "--train-list",
            str(corpus / "train.txt"), "--valid-list", str(corpus / "valid.txt"), "--outdir", str(outdir), "--sampling-rate", str(FS), "--generator-params",
            json.dumps(G_PARAMS), "--discriminator-params", json.dumps(D_PARAMS), "--mel-loss-params", json.dumps(MEL), "--batch-size", "3",
            "--batch-max-steps", "1280", "--discriminator-train-start-steps", "2", "--train-max-steps", "4", "--save-interval-steps", "2",
            "--eval-interval-steps", "2", "--log-interval-steps", "2", "--seed", "3", "--verbose", "0"] + list(more)


@pytest.fixture(scope="module")
def run4(TV, corpus, tmp_path_factory):  # noqa: F811
    out = tmp_path_factory.mktemp("hifigan_run4")
    TV.main(argv_of(corpus, out))
    return out


def test_four_steps_move_the_right_parameters_and_log_what_is_promised(TV, corpus, run4):  # noqa: F811
    ck2, _ = states(run4 / "checkpoint-2steps.pkl")
    ck4, _ = states(run4 / "checkpoint-4steps.pkl")
    assert ck2["steps"] == 2 and ck4["steps"] == 4 and ck4["epochs"] == 2
    first = TV.HiFiGANTrainer(TV.resolve(TV.build_parser().parse_args(argv_of(corpus, run4))), torch.device(DEV))  # the same seed: the initial weights
    g0, d0 = ({k: v.detach().cpu() for k, v in m.state_dict().items()} for m in (first.gen, first.disc))
    assert set(g0) == set(ck4["model"]["generator"]) and "input_conv.weight_g" in g0 and "msd.discriminators.0.layers.0.0.weight_orig" in d0
    for k, v in ck4["model"]["generator"].items():
        assert torch.isfinite(v).all() and not torch.equal(v, g0[k]), k
    for k, v in ck2["model"]["discriminator"].items():
        assert torch.equal(v, d0[k]), k  # not before step 3 (the spectral norm's buffers included: no forward in training mode ran)
    for k, v in ck4["model"]["discriminator"].items():
        # (the score layer's weight_u is a unit vector of ONE element: 1.0 whatever the power iteration does)
        assert torch.isfinite(v).all() and torch.equal(v, d0[k]) == (k.endswith("weight_u") and v.numel() == 1), k
    lines = [json.loads(ln) for ln in (run4 / "train_log.jsonl").read_text().splitlines()]
    assert lines[0] == {"left_out": ["short"]}
    logs, evals = [r for r in lines if "ms_per_step" in r], [r for r in lines if "eval_windows" in r]
    assert [r["step"] for r in logs] == [2, 4] and [r["step"] for r in evals] == [2, 4]
    keys = set(TERMS) | {"step", "generator_lr", "discriminator_lr", "generator_grad_norm", "discriminator_grad_norm", "ms_per_step", "samples_per_second"}
    for r in logs:
        assert set(r) == keys and r["generator_lr"] == 2e-4 and r["discriminator_lr"] == 2e-4
    assert all(logs[0][k] is None for k in TERMS[1:] + ("discriminator_grad_norm",))
    assert all(np.isfinite(v) for k, v in logs[0].items() if v is not None) and all(np.isfinite(v) for v in logs[1].values())
    assert set(evals[0]) == {"step", "eval_windows", "eval_mel_loss"} and evals[0]["eval_windows"] == 1
    assert set(evals[1]) == {"step", "eval_windows", "eval_mel_loss", "eval_adversarial_loss", "eval_feature_matching_loss"}
    assert all(np.isfinite(v) for v in evals[1].values())
    y = __import__("yaml").safe_load((run4 / "config.yml").read_text())
    assert y["generator_type"] == "HiFiGANGenerator" and y["hop_size"] == HOP and y["generator_params"]["channels"] == 256


def test_the_decoders_load_the_checkpoint(TV, corpus, run4, tmp_path):  # noqa: F811
    from fcl_taco2_amd import hifigan, vocoder_decode as VD
    from fcl_taco2_amd.kaldi_io import ArkScpWriter

    ckpt = str(run4 / "checkpoint-4steps.pkl")
    assert VD.generator_type(ckpt) == "HiFiGANGenerator"
    mel = np.load(corpus / "feats" / "mels" / "u4.npy")
    with ArkScpWriter(str(tmp_path / "feats")) as w:
        w["u4"] = mel
    samples, _ = VD.main(["--checkpoint", ckpt, "--feats-scp", str(tmp_path / "feats.scp"), "--outdir", str(tmp_path / "wav"), "--verbose", "0"])
    with wave.open(str(tmp_path / "wav" / "u4_gen.wav")) as f:
        assert (f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()) == (1, 2, FS, mel.shape[0] * HOP) and samples == mel.shape[0] * HOP
        pcm = np.frombuffer(f.readframes(f.getnframes()), dtype="<i2")
    assert np.abs(pcm).max() > 0
    ck = torch.load(ckpt, map_location="cpu", weights_only=True)
    cfg, rate = VD.hifigan_config(ckpt)
    gen = hifigan.HiFiGANGenerator(hifigan.HiFiGANPlan({k: v.numpy() for k, v in ck["model"]["generator"].items()}, DEV, cfg))
    wav = gen.synthesize([mel])[0]
    assert rate == FS and gen.plan.hop == HOP and wav.numel() == mel.shape[0] * HOP and bool(torch.isfinite(wav).all())


def test_resume_gives_the_bytes_of_the_uninterrupted_run(TV, corpus, run4, tmp_path):  # noqa: F811
    TV.main(argv_of(corpus, tmp_path, "--train-max-steps", "2"))
    TV.main(argv_of(corpus, tmp_path, "--resume", str(tmp_path / "checkpoint-2steps.pkl")))
    (_, a), (_, b) = states(run4 / "checkpoint-4steps.pkl"), states(tmp_path / "checkpoint-4steps.pkl")
    assert set(a) == set(b) and len([k for k in a if k.startswith("optimizer.discriminator")]) > 0
    for k in a:
        assert torch.equal(a[k], b[k]), k
    (_, a2), (_, b2) = states(run4 / "checkpoint-2steps.pkl"), states(tmp_path / "checkpoint-2steps.pkl")
    assert all(torch.equal(a2[k], b2[k]) for k in a2)
    with pytest.raises(ValueError, match="lambda_feat_match"):
        TV.main(argv_of(corpus, tmp_path, "--resume", str(tmp_path / "checkpoint-2steps.pkl"), "--lambda-feat-match", "1.0"))
    # --pretrain loads the models only: the step count starts over
    out = tmp_path / "pre"
    tr = TV.main(argv_of(corpus, out, "--pretrain", str(run4 / "checkpoint-4steps.pkl"), "--train-max-steps", "2"))
    assert tr.steps == 2 and (out / "checkpoint-2steps.pkl").exists()


def test_a_nan_in_a_mel_stops_the_run_naming_step_and_term(TV, corpus, tmp_path):  # noqa: F811
    import shutil

    bad = tmp_path / "feats" / "mels"
    shutil.copytree(corpus / "feats" / "mels", bad)
    m = np.load(bad / "u1.npy")
    m[:, 3] = np.nan
    np.save(bad / "u1.npy", m)
    argv = argv_of(corpus, tmp_path / "out")
    argv[argv.index("--feature-root") + 1] = str(tmp_path / "feats")
    with pytest.raises(FloatingPointError, match=r"step 1: (mel_loss|generator_grad_norm) is nan"):
        TV.main(argv)
    assert not list((tmp_path / "out").glob("checkpoint-*"))


def test_no_discriminator_weight_gradient_in_the_generators_adversarial_backward(TV, corpus, tmp_path):  # noqa: F811
    """by the launch record: the discriminators run forward and backward to their input, and none of their weight-gradient kernels is launched"""
    from test_gpu_pwg_generator import record

    tr = TV.HiFiGANTrainer(TV.resolve(TV.build_parser().parse_args(argv_of(corpus, tmp_path))), torch.device(DEV))
    c, wav = torch.randn(3, 16, 20, device=DEV), 0.3 * torch.randn(3, 1, 1280, device=DEV)
    dw = lambda seen: [k for k in seen if k.startswith(("hpd_dw", "hsd_dw"))]
    with record() as seen:
        _, terms = tr.losses(c, wav, True)
        assert set(terms) == {"mel_loss", "adversarial_loss", "feature_matching_loss"}
        assert all(p.requires_grad for p in tr.disc.parameters())  # released again before the backward pass
        tr.disc.zero_grad()
        sum(terms.values()).backward()
    assert [k for k in seen if k.startswith("hpd_")] and [k for k in seen if k.startswith("hsd_")] and not dw(seen), sorted(seen)
    assert "hfe_fwd_kernel" in seen and "hfe_dx_kernel" in seen and "hfe_dw_kernel" in seen  # the generator's output end ran in HIP
    assert all(p.grad is None for p in tr.disc.parameters()) and all(p.grad is not None for p in tr.gen.parameters())
    with record() as seen:  # (the control: the discriminator's own update does launch them)
        sum(out[-1].square().mean() for out in tr.disc(wav)).backward()
    assert dw(seen)


def test_three_steps_with_the_hip_end_against_the_torch_end(TV, corpus, tmp_path):  # noqa: F811
    """the same seed, 3 steps (the third with the adversarial and feature-matching terms), --output-end hip against --output-end torch, every step's
    terms from the log (interval 1): within the measured margin of the torch-end leg"""
    logs = {}
    for end in ("hip", "torch"):
        out = tmp_path / end
        argv = argv_of(corpus, out, "--output-end", end, "--train-max-steps", "3")
        argv[argv.index("--log-interval-steps") + 1] = "1"
        TV.main(argv)
        logs[end] = [r for r in (json.loads(ln) for ln in (out / "train_log.jsonl").read_text().splitlines()) if "ms_per_step" in r]
        assert [r["step"] for r in logs[end]] == [1, 2, 3]
    worst = {}
    for a, b in zip(logs["hip"], logs["torch"]):
        for name in TERMS:
            assert (a[name] is None) == (b[name] is None)
            if a[name] is not None:
                worst[(a["step"], name)] = abs(a[name] - b[name]) / abs(b[name])
    print("steps 1 - 3, relative differences against the torch-end leg: %s" % {k: float("%.3g" % v) for k, v in worst.items()})
    assert (3, "adversarial_loss") in worst and (3, "feature_matching_loss") in worst and (1, "mel_loss") in worst
    assert max(worst.values()) <= MARGIN, worst
