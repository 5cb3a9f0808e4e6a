"""CPU checks for python -m fcl_taco2_amd.train_vocoder: the parser's defaults are the published parallel_wavegan.v1 recipe, a config file round-trips
and an unknown key is refused by name, the window sampler stays inside its bounds, cuts corresponding mel and wav slices and is a function of (seed,
step) alone, the schedule (the first adversarial step, StepLR's values), the checkpoint's key layout, and the written config.yml read back by
vocoder_decode."""
import json
import os

import numpy as np
import pytest
import torch
import yaml


@pytest.fixture(scope="module")
def TV():
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import train_vocoder

    return train_vocoder


def args_of(TV, *argv):
    return TV.build_parser().parse_args(["--outdir", "unused"] + list(argv))


TINY_G = dict(layers=4, stacks=2, residual_channels=16, gate_channels=32, skip_channels=16, aux_channels=16, upsample_params={"upsample_scales": [4, 4, 4]})
TINY_D = dict(layers=4, conv_channels=16)


def test_defaults_are_the_published_v1_recipe(TV):
    cfg = TV.resolve(args_of(TV))
    assert (cfg["batch_size"], cfg["batch_max_steps"]) == (6, 25600)
    assert cfg["generator_optimizer_type"] == cfg["discriminator_optimizer_type"] == "RAdam"
    assert cfg["generator_optimizer_params"] == {"lr": 1e-4, "eps": 1e-6} and cfg["discriminator_optimizer_params"] == {"lr": 5e-5, "eps": 1e-6}
    assert cfg["generator_scheduler_params"] == cfg["discriminator_scheduler_params"] == {"step_size": 200000, "gamma": 0.5}
    assert (cfg["generator_grad_norm"], cfg["discriminator_grad_norm"], cfg["lambda_adv"]) == (10.0, 1.0, 4.0)
    assert (cfg["discriminator_train_start_steps"], cfg["train_max_steps"]) == (100000, 400000)
    assert (cfg["save_interval_steps"], cfg["eval_interval_steps"], cfg["log_interval_steps"]) == (5000, 1000, 100)
    assert cfg["stft_loss_params"] == {"fft_sizes": [1024, 2048, 512], "hop_sizes": [120, 240, 50], "win_lengths": [600, 1200, 240]}
    g, d = cfg["generator_params"], cfg["discriminator_params"]
    assert (g["layers"], g["stacks"], g["residual_channels"], g["aux_channels"], g["aux_context_window"]) == (30, 3, 64, 80, 2)
    assert g["upsample_params"] == {"upsample_scales": [4, 4, 4, 4]} and cfg["hop_size"] == 256 and (d["layers"], d["conv_channels"]) == (10, 64)
    # every one is a flag
    cfg = TV.resolve(args_of(TV, "--batch-size", "3", "--generator-lr", "2e-4", "--fft-sizes", "512,512", "--hop-sizes", "50 30", "--win-lengths", "240,120",
                             "--generator-params", json.dumps(TINY_G), "--discriminator-params", json.dumps(TINY_D), "--batch-max-steps", "1280", "--seed", "5"))
    assert cfg["batch_size"] == 3 and cfg["generator_optimizer_params"]["lr"] == 2e-4 and cfg["stft_loss_params"]["hop_sizes"] == [50, 30]
    assert cfg["hop_size"] == 64 and cfg["generator_params"]["layers"] == 4 and cfg["discriminator_params"]["conv_channels"] == 16 and cfg["seed"] == 5


def test_config_round_trips_and_unknown_keys_are_refused_by_name(TV, tmp_path):
    cfg = TV.resolve(args_of(TV, "--generator-params", json.dumps(TINY_G), "--discriminator-params", json.dumps(TINY_D), "--batch-max-steps", "1280",
                             "--lambda-adv", "2.5", "--seed", "9"))
    path = tmp_path / "config.yml"
    path.write_text(yaml.safe_dump(json.loads(json.dumps(cfg))))
    assert TV.resolve(args_of(TV, "--config", str(path))) == cfg
    assert TV.resolve(args_of(TV, "--config", str(path), "--lambda-adv", "1.0"))["lambda_adv"] == 1.0  # a flag beside the file wins
    assert TV.resolve(args_of(TV, "--config", str(path)))["seed"] == 9 and TV.resolve(args_of(TV, "--config", str(path), "--seed", "0"))["seed"] == 0
    assert TV.resolve(args_of(TV))["seed"] == 0
    # every refused key of a file is named in the one message (a real parallel_wavegan config carries many the driver has no use for)
    y = json.loads(json.dumps(cfg))
    y.update(fft_size=1024, num_mels=80, format="hdf5", trim_silence=False)
    y["generator_optimizer_params"]["weight_decay"] = 0.0
    path.write_text(yaml.safe_dump(y))
    with pytest.raises(ValueError) as e:
        TV.resolve(args_of(TV, "--config", str(path)))
    assert all(k in str(e.value) for k in ("fft_size", "num_mels", "format", "trim_silence", "generator_optimizer_params.weight_decay"))
    for where, key in ((None, "use_noise_shaping"), ("generator_params", "use_pixel_shuffle"), ("discriminator_params", "periods"),
                       ("stft_loss_params", "window"), ("generator_optimizer_params", "weight_decay"), ("generator_scheduler_params", "milestones")):
        y = json.loads(json.dumps(cfg))
        (y if where is None else y[where])[key] = 1
        path.write_text(yaml.safe_dump(y))
        with pytest.raises(ValueError, match=key):
            TV.resolve(args_of(TV, "--config", str(path)))
    y = json.loads(json.dumps(cfg))
    y["generator_type"] = "MelGANGenerator"
    path.write_text(yaml.safe_dump(y))
    with pytest.raises(ValueError, match="generator_type"):
        TV.resolve(args_of(TV, "--config", str(path)))
    with pytest.raises(ValueError, match="batch_max_steps"):
        TV.resolve(args_of(TV, "--batch-max-steps", "1000"))
    with pytest.raises(ValueError, match="upsample_scales"):
        TV.resolve(args_of(TV, "--generator-params", json.dumps(dict(TINY_G, upsample_params={"upsample_scales": [32]}))))


def test_window_sampler(TV):
    frames, ctx, hop = 20, 2, 64
    lengths = [("a", 24), ("b", 30), ("short", 23), ("c", 100), ("d", 57)]
    s = TV.Windows(lengths, frames, ctx, hop, 3, seed=11)
    assert s.dropped == ["short"] and [u for u, _ in s.utts] == ["a", "b", "c", "d"]
    seen = set()
    for step in range(1, 200):
        for k, f0 in s.batch(step):
            T = s.utts[k][1]
            assert ctx <= f0 <= T - ctx - frames
            seen.add((k, f0))
            mel, wav = np.arange(T * 4).reshape(T, 4), np.arange((T - 1) * hop)
            m, w = s.cut(mel, wav, f0)
            assert m.shape == (frames + 2 * ctx, 4) and w.shape == (frames * hop,) and w[0] == f0 * hop and m[0, 0] == (f0 - ctx) * 4
    assert {k for k, _ in seen} == {0, 1, 2, 3} and (0, 2) in seen and {f for k, f in seen if k == 1} == set(range(2, 9))  # both ends of every range are reached
    # every epoch visits every utterance once
    flat = [k for step in range(1, 9) for k, _ in s.batch(step)]
    assert all(sorted(flat[i : i + 4]) == [0, 1, 2, 3] for i in range(0, 24, 4)) and s.epoch(1) == 0 and s.epoch(2) == 1 and s.epoch(4) == 2
    # a function of (seed, step) alone: two samplers asked in different orders agree
    a, b = TV.Windows(lengths, frames, ctx, hop, 3, seed=11), TV.Windows(lengths, frames, ctx, hop, 3, seed=11)
    for step in (3, 9, 7):
        a.batch(step), a.noise(step)
    assert a.batch(7) == b.batch(7) and np.array_equal(a.noise(7), b.noise(7)) and a.noise(7).dtype == np.float32 and a.noise(7).shape == (3, 1, frames * hop)
    assert a.batch(7) != TV.Windows(lengths, frames, ctx, hop, 3, seed=12).batch(7) and not np.array_equal(a.noise(7), a.noise(8))
    f0, z = a.valid(2)
    assert f0 == b.valid(2)[0] and np.array_equal(z, b.valid(2)[1]) and ctx <= f0 <= 100 - ctx - frames
    with pytest.raises(ValueError, match="no utterance is long enough.*short"):
        TV.Windows([("short", 23), ("tiny", 3)], frames, ctx, hop, 3, seed=0)


def test_schedule(TV):
    cfg = TV.resolve(args_of(TV))
    assert not TV.adversarial(cfg, 100000) and TV.adversarial(cfg, 100001)
    assert TV.learning_rate(cfg, "generator", 199999) == 1e-4 and TV.learning_rate(cfg, "generator", 200000) == 1e-4
    assert TV.learning_rate(cfg, "generator", 200001) == 5e-5 and TV.learning_rate(cfg, "discriminator", 400001) == 5e-5 * 0.25
    # ... which is torch's StepLR: after 199 999 scheduler steps the rate is the first, after 200 000 it is halved
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.RAdam([p], lr=1e-4, eps=1e-6)
    sch = torch.optim.lr_scheduler.StepLR(opt, step_size=200000, gamma=0.5)
    sch.last_epoch = 199998
    opt.step(), sch.step()
    assert sch.last_epoch == 199999 and opt.param_groups[0]["lr"] == 1e-4
    opt.step(), sch.step()
    assert sch.last_epoch == 200000 and opt.param_groups[0]["lr"] == 5e-5
    small = TV.resolve(args_of(TV, "--scheduler-step-size", "3"))
    q = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.RAdam([q], lr=1e-4, eps=1e-6)
    sch = torch.optim.lr_scheduler.StepLR(opt, step_size=3, gamma=0.5)
    for step in range(1, 11):
        assert opt.param_groups[0]["lr"] == pytest.approx(TV.learning_rate(small, "generator", step), rel=1e-12)
        opt.step(), sch.step()


def test_checkpoint_layout_and_config_read_back_by_the_decoder(TV, tmp_path):
    """the modules construct on the CPU (only their forward needs the device)"""
    from fcl_taco2_amd import vocoder_decode
    from fcl_taco2_amd.pwg_discriminator import ParallelWaveGANDiscriminator
    from fcl_taco2_amd.pwg_generator import TrainableParallelWaveGANGenerator

    cfg = TV.resolve(args_of(TV, "--generator-params", json.dumps(TINY_G), "--discriminator-params", json.dumps(TINY_D), "--batch-max-steps", "1280",
                             "--sampling-rate", "16000"))
    gen, disc = TrainableParallelWaveGANGenerator(**cfg["generator_params"]), ParallelWaveGANDiscriminator(**cfg["discriminator_params"])
    opt = {"generator": torch.optim.RAdam(gen.parameters(), **cfg["generator_optimizer_params"]),
           "discriminator": torch.optim.RAdam(disc.parameters(), **cfg["discriminator_optimizer_params"])}
    sch = {k: torch.optim.lr_scheduler.StepLR(opt[k], **cfg[k + "_scheduler_params"]) for k in opt}
    ck = TV.checkpoint_of(gen, disc, opt, sch, 4, 1)
    assert set(ck) == {"model", "optimizer", "scheduler", "steps", "epochs"} and ck["steps"] == 4 and ck["epochs"] == 1
    assert all(set(ck[k]) == {"generator", "discriminator"} for k in ("model", "optimizer", "scheduler"))
    assert "first_conv.weight_g" in ck["model"]["generator"] and "conv_layers.0.weight_v" in ck["model"]["discriminator"]
    path = tmp_path / "checkpoint-4steps.pkl"
    torch.save(ck, path)
    back = torch.load(path, weights_only=True)  # tensors and plain containers only: what vocoder_decode.load_checkpoint accepts
    assert set(back["optimizer"]["generator"]) == {"state", "param_groups"} and back["scheduler"]["generator"]["step_size"] == 200000
    assert set(vocoder_decode.load_checkpoint(str(path))["model"]) == {"generator"}
    (tmp_path / "config.yml").write_text(yaml.safe_dump(json.loads(json.dumps(cfg)), sort_keys=False))
    got, rate = vocoder_decode.generator_config(str(path))
    assert rate == 16000 and got == dict(layers=4, stacks=2, residual_channels=16, gate_channels=32, skip_channels=16, aux_channels=16, aux_context_window=2,
                                         kernel_size=3, upsample_scales=(4, 4, 4))
    assert vocoder_decode.generator_type(str(path)) == "ParallelWaveGANGenerator"
    y = yaml.safe_load((tmp_path / "config.yml").read_text())
    assert vocoder_decode._pwg_config_of(y)[0]["upsample_scales"] == (4, 4, 4) and y["hop_size"] == 64
    # a resume under other values is refused naming the key
    TV.check_resume(cfg, str(path))
    with pytest.raises(ValueError, match="batch_size"):
        TV.check_resume(dict(cfg, batch_size=4), str(path))
    with pytest.raises(ValueError, match="generator_optimizer_params"):
        TV.check_resume(dict(cfg, generator_optimizer_params={"lr": 3e-4, "eps": 1e-6}), str(path))
