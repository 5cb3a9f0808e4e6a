"""HiFi-GAN generator, the parts that need no GPU: the parameter table, weight-norm folding of a transposed layer, the transposed convolution's
index rule against torch, the `generator_type` dispatch of vocoder_decode, and -- with the float64 reference alone (tests/hifigan_ref.py) -- the
conditions under which the GPU tests' inputs exercise the generator (tests/test_gpu_hifigan.py uses the very same arrays)."""
import logging
import os

import numpy as np
import pytest
import torch

import hifigan_ref as R


def test_param_spec_v1_is_the_published_table():
    from fcl_taco2_amd import hifigan

    spec = hifigan.param_spec()
    assert len(spec) == 2 + 4 * 2 + 12 * 3 * 2 * 2 + 2
    assert spec["input_conv.weight"] == (512, 80, 7) and spec["input_conv.bias"] == (512,)
    for i, (ci, ku) in enumerate(((512, 16), (256, 16), (128, 4), (64, 4))):
        assert spec["upsamples.%d.1.weight" % i] == (ci, ci // 2, ku)  # ConvTranspose1d: dim 0 is the INPUT channel
        assert spec["upsamples.%d.1.bias" % i] == (ci // 2,)
        for j, kr in enumerate((3, 7, 11)):
            for d in range(3):
                for cv in ("convs1", "convs2"):
                    p = "blocks.%d.%s.%d.1." % (i * 3 + j, cv, d)
                    assert spec[p + "weight"] == (ci // 2, ci // 2, kr) and spec[p + "bias"] == (ci // 2,)
    assert spec["output_conv.1.weight"] == (1, 32, 7) and spec["output_conv.1.bias"] == (1,)
    assert list(spec) == list(R.param_shapes(R.V1)) and all(spec[k] == R.param_shapes(R.V1)[k][0] for k in spec)
    small = hifigan.param_spec(R.plan_cfg(R.SMALL))
    assert {k: v for k, v in small.items()} == {k: v[0] for k, v in R.param_shapes(R.SMALL).items()}


def test_weight_norm_folding_of_a_transposed_layer_is_torchs():
    """torch.nn.utils.weight_norm's default dim = 0 norms over every dimension but 0 -- for a ConvTranspose1d that is per INPUT channel"""
    from fcl_taco2_amd import vocoder

    torch.manual_seed(3)
    layer = torch.nn.utils.weight_norm(torch.nn.ConvTranspose1d(6, 4, 8, stride=4, padding=2))
    with torch.no_grad():
        layer.weight_g.mul_(torch.rand_like(layer.weight_g) + 0.5)
    sd = {"upsamples.0.1." + k: v.detach().numpy() for k, v in layer.state_dict().items()}
    assert set(sd) == {"upsamples.0.1.bias", "upsamples.0.1.weight_g", "upsamples.0.1.weight_v"} and sd["upsamples.0.1.weight_g"].shape == (6, 1, 1)
    want = torch._weight_norm(layer.weight_v, layer.weight_g, 0).detach().numpy()
    got = vocoder.fold_weight_norm(sd)
    assert set(got) == {"upsamples.0.1.bias", "upsamples.0.1.weight"}
    np.testing.assert_allclose(got["upsamples.0.1.weight"], want, rtol=0, atol=2e-7 * float(np.abs(want).max()))


@pytest.mark.parametrize("s", [2, 4, 8])
def test_tconv_index_rule_is_conv_transpose1d(s):
    from fcl_taco2_amd import hifigan

    rng = np.random.RandomState(40 + s)
    cin, cout, ku = 5, 3, 2 * s
    w, b = rng.standard_normal((cin, cout, ku)), rng.standard_normal(cout)
    for lens in ([1], [1, 1, 1], [3, 1, 7, 2], [2, 9]):
        x = rng.standard_normal((sum(lens), cin))
        got = hifigan.tconv_rule(x, w, b, s, lens)
        want, off = [], 0
        for n in lens:
            want.append(R.tconv(R.f64(x[off : off + n]), R.f64(w), R.f64(b), s).numpy())
            off += n
        want = np.concatenate(want)
        assert got.shape == want.shape == (sum(lens) * s, cout)
        assert np.max(np.abs(got - want)) <= 1e-12 * max(1.0, float(np.abs(want).max())), (s, lens)
    with pytest.raises(ValueError, match="multiple of the stride"):
        hifigan.tconv_rule(np.zeros((2, cin)), np.zeros((cin, cout, 2 * s + 1)), b, s, [2])


def write_cfg(tmp_path, text):
    d = tmp_path / ("c%d" % len(list(tmp_path.iterdir())))
    d.mkdir()
    (d / "config.yml").write_text(text)
    return str(d / "checkpoint.pkl")


HFG_YML = """sampling_rate: 24000
generator_type: HiFiGANGenerator
generator_params:
  in_channels: 80
  out_channels: 1
  channels: 128
  kernel_size: 7
  upsample_scales: [4, 2]
  upsample_kernel_sizes: [8, 4]
  resblock_kernel_sizes: [3, 7, 11]
  resblock_dilations: [[1, 3, 5], [1, 3, 5], [1, 3, 5]]
  use_additional_convs: true
  bias: true
  nonlinear_activation: LeakyReLU
  nonlinear_activation_params: {negative_slope: 0.1}
  use_weight_norm: true
"""


def test_generator_type_dispatch(tmp_path):
    from fcl_taco2_amd import hifigan, vocoder_decode as V

    pwg_yml = "sampling_rate: 16000\ngenerator_params:\n  layers: 6\n  stacks: 3\n  upsample_params:\n    upsample_scales: [4, 4, 4]\n"
    for text in (pwg_yml, "generator_type: ParallelWaveGANGenerator\n" + pwg_yml):
        ck = write_cfg(tmp_path, text)
        assert V.generator_type(ck) == "ParallelWaveGANGenerator"
        assert V.generator_config(ck) == ({"layers": 6, "stacks": 3, "upsample_scales": (4, 4, 4)}, 16000)  # today's result, unchanged
    assert V.generator_type(str(tmp_path / "nowhere" / "ck.pkl")) is None and V.generator_config(str(tmp_path / "nowhere" / "ck.pkl")) == ({}, 22050)
    ck = write_cfg(tmp_path, HFG_YML)
    assert V.generator_type(ck) == "HiFiGANGenerator"
    cfg, rate = V.hifigan_config(ck)
    assert rate == 24000 and hifigan.config(cfg)["upsample_scales"] == (4, 2) and hifigan.config(cfg)["channels"] == 128
    assert hifigan.param_spec(cfg) == {k: v[0] for k, v in R.param_shapes(R.SMALL).items()}
    ck = write_cfg(tmp_path, "generator_type: MelGANGenerator\n")
    with pytest.raises(NotImplementedError, match="MelGANGenerator"):
        V.build_generator(ck, "cuda:0")  # refused before the checkpoint is read or a device is touched


@pytest.mark.parametrize("line,name", [
    ("  nonlinear_activation: LeakyReLU", "  nonlinear_activation: ReLU"), ("  use_additional_convs: true", "  use_additional_convs: false"),
    ("  bias: true", "  bias: false"), ("  upsample_kernel_sizes: [8, 4]", "  upsample_kernel_sizes: [6, 4]"),
    ("  upsample_kernel_sizes: [8, 4]", "  upsample_kernel_sizes: [16, 4]"), ("  resblock_kernel_sizes: [3, 7, 11]", "  resblock_kernel_sizes: [3, 7, 13]"),
    ("  channels: 128", "  channels: 64"), ("  use_weight_norm: true", "  use_causal_conv: true")])
def test_unsupported_generator_params_are_refused_by_name(tmp_path, line, name):
    from fcl_taco2_amd import vocoder_decode as V

    assert line in HFG_YML
    ck = write_cfg(tmp_path, HFG_YML.replace(line, name))
    with pytest.raises(NotImplementedError, match=name.split(":")[0].strip()):
        V.hifigan_config(ck)


def test_family_and_geometry_from_the_state_dict_without_a_config(caplog):
    from fcl_taco2_amd import hifigan, vocoder, vocoder_decode as V

    sd = R.random_state_dict(np.random.RandomState(1), R.SMALL)
    for form in (sd, R.with_weight_norm(sd, np.random.RandomState(2)), {"model": {"generator": sd}}):
        assert V.family_of_state_dict(form) == "HiFiGANGenerator"
        with caplog.at_level(logging.WARNING):
            caplog.clear()
            cfg, rate = V.hifigan_config_from_shapes(form)
        assert "ASSUMING" in caplog.text and "(1, 3, 5)" in caplog.text  # the assumption is logged
        assert rate == 22050 and hifigan.param_spec(cfg) == {k: v[0] for k, v in R.param_shapes(R.SMALL).items()}
    pwg = {k: np.zeros(s, np.float32) for k, s in vocoder.param_spec().items()}
    assert V.family_of_state_dict(pwg) == "ParallelWaveGANGenerator" and V.family_of_state_dict({"model": {"generator": pwg}}) == "ParallelWaveGANGenerator"
    with pytest.raises(NotImplementedError, match="unknown generator family"):
        V.family_of_state_dict({"conv.weight": np.zeros(3)})
    folded = vocoder.fold_weight_norm(R.with_weight_norm(sd, np.random.RandomState(2)))
    for k in sd:
        np.testing.assert_allclose(folded[k], sd[k], rtol=0, atol=1e-6 * float(np.abs(sd[k]).max()))


def test_loader_names_the_first_offender():
    from fcl_taco2_amd import _lib, hifigan

    cfg = hifigan.config(R.plan_cfg(R.SMALL))
    sd = R.random_state_dict(np.random.RandomState(1), R.SMALL)
    hifigan.check_state_dict(sd, cfg)
    bad = dict(sd)
    bad["upsamples.1.1.weight"] = np.transpose(sd["upsamples.1.1.weight"], (1, 0, 2))  # (out, in, k): a Conv1d layout
    with pytest.raises(_lib.FclError, match=r"upsamples\.1\.1\.weight \(64, 32, 4\)"):
        hifigan.check_state_dict(bad, cfg)
    bad = {k: v for k, v in sd.items() if k != "blocks.4.convs2.1.1.bias"}
    with pytest.raises(_lib.FclError, match=r"lacks blocks\.4\.convs2\.1\.1\.bias"):
        hifigan.check_state_dict(bad, cfg)
    with pytest.raises(_lib.FclError, match="first_conv.weight"):
        hifigan.check_state_dict(dict(sd, **{"first_conv.weight": np.zeros((1,))}), cfg)
    with pytest.raises(_lib.FclError, match="GPU"):
        hifigan.HiFiGANPlan(sd, "cpu", R.plan_cfg(R.SMALL))


@pytest.mark.parametrize("key", ["small", "v1"])
def test_gpu_test_inputs_exercise_the_generator(key):
    """With the reference alone, on the arrays the GPU tests use: every LeakyReLU sees 30 - 70 % negative arguments, |pre-tanh| < 4 everywhere (tanh
    hides nothing), and taking any single residual unit out moves the waveform by at least 1000 x the bound the GPU test asserts."""
    torch.set_num_threads(min(16, max(1, os.cpu_count() or 1)))
    cfg = dict(v1=R.V1, small=R.SMALL)[key]
    sd, mels = R.generator_inputs(R.SEEDS[key], R.GENERATOR_LENS, cfg)
    runs = [R.generator_f64(sd, m, cfg) for m in mels]
    n_sites = len(runs[0]["lrelu_args"])
    assert n_sites == len(cfg["upsample_scales"]) * (1 + 2 * len(R.units_of(cfg)) // len(cfg["upsample_scales"])) + 1
    fracs = []
    for i in range(n_sites):
        a = torch.cat([r["lrelu_args"][i].reshape(-1) for r in runs])
        fracs.append(float((a < 0).double().mean()))
    peak = max(float(r["pre"].abs().max()) for r in runs)
    print("%s: negative LeakyReLU arguments %.1f - %.1f %%, pre-tanh peak %.2f" % (key, 100 * min(fracs), 100 * max(fracs), peak))
    assert 0.30 <= min(fracs) and max(fracs) <= 0.70, fracs
    assert peak < 4.0
    sd1, mel1 = R.generator_inputs(R.SEEDS[key], R.CONDITION_LENS[key], cfg)
    assert all(np.array_equal(sd[k], sd1[k]) for k in sd)
    ref = R.generator_f64(sd1, mel1[0], cfg)
    mod = R.generator_f64(sd1, mel1[0], cfg, rnd=R.plane_round)
    e_mod = float((mod["wav"] - ref["wav"]).abs().max())
    bound = R.bound(e_mod, float(ref["wav"].abs().max()))
    effects = [float((R.generator_f64(sd1, mel1[0], cfg, zero_unit=u)["wav"] - ref["wav"]).abs().max()) for u in R.units_of(cfg)]
    print("%s: model error %.3e, bound %.3e, smallest single-unit effect %.3e" % (key, e_mod, bound, min(effects)))
    assert min(effects) >= 1000 * bound, (min(effects), bound)
