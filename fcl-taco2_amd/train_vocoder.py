"""Vocoder training on MI355X, two recipes chosen by generator_type (--generator-type, or the key of --config).

ParallelWaveGANGenerator (the default): the published parallel_wavegan.v1 recipe (restated from its paper and config, not diffed against a file): the
generator step is HIP from (z, c) to the waveform and back (pwg_generator.py), the discriminator and the multi-resolution STFT loss
are §6l and §6j.  HiFiGANGenerator: the published hifigan.v1 recipe (restated from the paper and the package's published configuration, not diffed
against a file, like the other): the generator is hifigan_generator.py with its output end in HIP (§6p, §6s), the discriminator the multi-scale +
multi-period one (§6q, §6r), the losses 45 x the mel-spectrogram L1 (§6k) + the MSE adversarial term + 2 x feature matching, Adam and MultiStepLR.
Torch keeps weight and spectral norm, the optimisers and the schedulers.

    python -m fcl_taco2_amd.train_vocoder --wav-dir wavs --feature-root feats --train-list train.txt --valid-list valid.txt --outdir exp/pwg
    python -m fcl_taco2_amd.train_vocoder --generator-type HiFiGANGenerator --wav-dir wavs ... --outdir exp/hifigan

reads `feats/mels/<utt>.npy` (the normalised [T, n_mels] mels that preprocess / extract_features write, T = samples // hop + 1) and 16-bit PCM mono wavs,
and writes config.yml (parallel_wavegan's layout), checkpoint-<steps>steps.pkl (vocoder.PWGPlan or hifigan.HiFiGANPlan, vocoder_decode and tts load
them as they are) and train_log.jsonl into --outdir.  Which utterances and windows make step n's batch, and the noise of step n, are functions of
(--seed, n) alone, so --resume needs nothing but the checkpoint: 2 + 2 steps give the bytes of 4.

    python -m fcl_taco2_amd.train_vocoder --gpus 8 ... --outdir exp/hifigan

trains data-parallel on one node (vocoder_dp.py): the command starts its ranks itself, or runs as one rank under torch.distributed.run.
--batch-size stays the GLOBAL batch -- rank r takes items i % W == r of step n's batch and of its noise, so a W-rank run consumes the batches, epochs and
step counts of the one-GPU run and a checkpoint does not pin the world size (parallel_wavegan's own batch_size is per process: for that meaning pass
16 * N).  Every rank takes its loss on its own shard and the ranks average their gradients, as DDP does; rank 0 alone writes the files.  A world of one
(without GradBuckets' FCL_DP_FORCE_COLLECTIVE) is the one-process step as it was."""
import argparse
import concurrent.futures
import json
import logging
import math
import os
import time

import numpy as np
import torch

from . import extract_features as XF

# the published v1 recipe; every one is a flag
DEFAULTS = dict(sampling_rate=22050, batch_size=6, batch_max_steps=25600, generator_lr=1e-4, discriminator_lr=5e-5, optimizer_eps=1e-6,
                scheduler_step_size=200000, scheduler_gamma=0.5, generator_grad_norm=10.0, discriminator_grad_norm=1.0, lambda_adv=4.0,
                discriminator_train_start_steps=100000, train_max_steps=400000, save_interval_steps=5000, eval_interval_steps=1000, log_interval_steps=100,
                fft_sizes=(1024, 2048, 512), hop_sizes=(120, 240, 50), win_lengths=(600, 1200, 240))
GENERATOR_DEFAULTS = dict(in_channels=1, out_channels=1, kernel_size=3, layers=30, stacks=3, residual_channels=64, gate_channels=128, skip_channels=64,
                          aux_channels=80, aux_context_window=2, dropout=0.0, bias=True, use_weight_norm=True, use_causal_conv=False,
                          upsample_conditional_features=True, upsample_net="ConvInUpsampleNetwork", upsample_params={"upsample_scales": [4, 4, 4, 4]})
DISCRIMINATOR_DEFAULTS = dict(in_channels=1, out_channels=1, kernel_size=3, layers=10, conv_channels=64, dilation_factor=1, bias=True, use_weight_norm=True,
                              nonlinear_activation="LeakyReLU", nonlinear_activation_params={"negative_slope": 0.2})
# a checkpoint is resumed only under the values it was trained with: these keys of config.yml must agree with the flags
PINNED = ("generator_params", "discriminator_params", "batch_size", "batch_max_steps", "generator_optimizer_params", "discriminator_optimizer_params",
          "generator_scheduler_params", "discriminator_scheduler_params", "generator_grad_norm", "discriminator_grad_norm", "lambda_adv",
          "discriminator_train_start_steps", "stft_loss_params", "sampling_rate", "hop_size", "seed", "generator_type", "discriminator_type",
          "mel_loss_params", "lambda_aux", "lambda_feat_match")  # (a key the recipe does not have is absent on both sides)
LOSS_TERMS = ("spectral_convergence_loss", "log_stft_magnitude_loss", "adversarial_loss", "real_loss", "fake_loss")
MAX_RANKS = 16  # of one job: no more processes than that hold a GPU at a time
PWG_TYPE, HIFIGAN_TYPE, HIFIGAN_DISCRIMINATOR = "ParallelWaveGANGenerator", "HiFiGANGenerator", "HiFiGANMultiScaleMultiPeriodDiscriminator"

# ---- the published hifigan.v1 recipe
HIFIGAN_DEFAULTS = dict(sampling_rate=22050, batch_size=16, batch_max_steps=8192, generator_grad_norm=-1.0, discriminator_grad_norm=-1.0, lambda_aux=45.0,
                        lambda_adv=1.0, lambda_feat_match=2.0, generator_train_start_steps=1, discriminator_train_start_steps=0, train_max_steps=2500000,
                        save_interval_steps=10000, eval_interval_steps=1000, log_interval_steps=100)
HIFIGAN_OPTIMIZER = dict(lr=2e-4, betas=[0.5, 0.9], weight_decay=0.0)
HIFIGAN_SCHEDULER = dict(gamma=0.5, milestones=[200000, 400000, 600000, 800000])
HIFIGAN_MEL_LOSS = dict(fs=22050, fft_size=1024, hop_size=256, win_length=None, num_mels=80, fmin=0, fmax=None, log_base=None)  # fmax null: fs / 2
HIFIGAN_GENERATOR_DEFAULTS = dict(in_channels=80, out_channels=1, channels=512, kernel_size=7, upsample_scales=[8, 8, 2, 2],
                                  upsample_kernel_sizes=[16, 16, 4, 4], resblock_kernel_sizes=[3, 7, 11], resblock_dilations=[[1, 3, 5], [1, 3, 5], [1, 3, 5]],
                                  use_additional_convs=True, bias=True, nonlinear_activation="LeakyReLU", nonlinear_activation_params={"negative_slope": 0.1},
                                  use_weight_norm=True)
_ACT = dict(nonlinear_activation="LeakyReLU", nonlinear_activation_params={"negative_slope": 0.1})
HIFIGAN_SCALE_DEFAULTS = dict(in_channels=1, out_channels=1, kernel_sizes=[15, 41, 5, 3], channels=128, max_downsample_channels=1024, max_groups=16, bias=True,
                              downsample_scales=[2, 2, 4, 4, 1], use_weight_norm=True, use_spectral_norm=False, **_ACT)
HIFIGAN_PERIOD_DEFAULTS = dict(in_channels=1, out_channels=1, kernel_sizes=[5, 3], channels=32, downsample_scales=[3, 3, 3, 3, 1],
                               max_downsample_channels=1024, bias=True, use_weight_norm=True, use_spectral_norm=False, **_ACT)
HIFIGAN_DISCRIMINATOR_DEFAULTS = dict(scales=3, scale_downsample_pooling="AvgPool1d", scale_downsample_pooling_params={"kernel_size": 4, "stride": 2, "padding": 2},
                                      scale_discriminator_params=HIFIGAN_SCALE_DEFAULTS, follow_official_norm=True, periods=[2, 3, 5, 7, 11],
                                      period_discriminator_params=HIFIGAN_PERIOD_DEFAULTS)


def _ints(text):
    return tuple(int(v) for v in str(text).replace(",", " ").split())


def _params(text, what):
    """constructor arguments as JSON or as a yaml file"""
    if text is None:
        return {}
    if os.path.exists(text):
        import yaml

        with open(text) as f:
            out = yaml.safe_load(f) or {}
    else:
        out = json.loads(text)
    if not isinstance(out, dict):
        raise ValueError("fcl-taco2_amd: train_vocoder: %s must be a mapping of constructor arguments, got %r" % (what, out))
    return out


def build_parser():
    d = DEFAULTS
    ap = argparse.ArgumentParser(prog="fcl_taco2_amd.train_vocoder",
                                 description="Vocoder training on MI355X: the parallel_wavegan.v1 recipe, or hifigan.v1 with --generator-type HiFiGANGenerator")
    ap.add_argument("--generator-type", default=None, help="%s (default) or %s: the recipe; also read from --config" % (PWG_TYPE, HIFIGAN_TYPE))
    ap.add_argument("--wav-dir", default=None, help="directory of <utt>.wav (16-bit PCM mono at --sampling-rate); this or --wav-scp")
    ap.add_argument("--wav-scp", default=None, help="Kaldi-style `utt path` list")
    ap.add_argument("--feature-root", default=None, help="reads mels/<utt>.npy: normalised [T, n_mels] mels as preprocess / extract_features write them")
    ap.add_argument("--train-list", default=None, help="utterance ids, one per line")
    ap.add_argument("--valid-list", default=None, help="utterance ids for the evaluation lines (optional)")
    ap.add_argument("--outdir", default=None)
    ap.add_argument("--gpus", type=int, default=1, help="data-parallel ranks on this node, one process each (at most %d); --batch-size stays the GLOBAL batch" % MAX_RANKS)
    ap.add_argument("--dist-backend", choices=("nccl", "gloo"), default="nccl", help="nccl: RCCL, one GPU per rank; gloo: ranks may share a GPU")
    ap.add_argument("--dist-timeout", type=float, default=600.0, help="seconds a collective waits for a rank before the job ends (default 600)")
    ap.add_argument("--dry-run-launch", action="store_true", help="rendezvous over gloo and one all-reduce of ones; rank 0 prints one JSON line; no device work")
    ap.add_argument("--config", default=None, help="parallel_wavegan-style config.yml for everything below; flags given beside it win")
    ap.add_argument("--generator-params", default=None, help="the trainable generator's constructor arguments, JSON or a yaml file (v1 without)")
    ap.add_argument("--discriminator-params", default=None, help="the discriminator's constructor arguments, JSON or a yaml file (v1 without)")
    ap.add_argument("--sampling-rate", type=int, default=None, help="default %d" % d["sampling_rate"])
    for k in ("batch_size", "batch_max_steps", "scheduler_step_size", "discriminator_train_start_steps", "train_max_steps", "save_interval_steps",
              "eval_interval_steps", "log_interval_steps"):
        ap.add_argument("--" + k.replace("_", "-"), type=int, default=None, help="default %d%s" % (d[k], " (Parallel WaveGAN only)" * (k == "scheduler_step_size")))
    for k in ("generator_lr", "discriminator_lr", "optimizer_eps", "scheduler_gamma", "generator_grad_norm", "discriminator_grad_norm", "lambda_adv"):
        ap.add_argument("--" + k.replace("_", "-"), type=float, default=None, help="default %g" % d[k])
    for k in ("fft_sizes", "hop_sizes", "win_lengths"):
        ap.add_argument("--" + k.replace("_", "-"), type=_ints, default=None, help="STFT loss resolutions, default %s" % ",".join(map(str, d[k])))
    ap.add_argument("--seed", type=int, default=None, help="default 0; of the batches, the windows and the noise (functions of the seed and the step alone)")
    ap.add_argument("--resume", default=None, help="checkpoint-Nsteps.pkl: continue with models, optimisers, schedulers and the step count")
    ap.add_argument("--pretrain", default=None, help="checkpoint.pkl: load the models only")
    ap.add_argument("--ends", choices=("hip", "torch"), default=None, help="Parallel WaveGAN: the generator's ends (DESIGN §6o), default hip")
    ap.add_argument("--output-end", choices=("hip", "torch"), default=None, help="HiFi-GAN: the generator's output end (DESIGN §6s), default hip")
    ap.add_argument("--lambda-aux", type=float, default=None, help="HiFi-GAN: the mel term's weight, default %g" % HIFIGAN_DEFAULTS["lambda_aux"])
    ap.add_argument("--lambda-feat-match", type=float, default=None,
                    help="HiFi-GAN: the feature-matching term's weight, default %g" % HIFIGAN_DEFAULTS["lambda_feat_match"])
    ap.add_argument("--mel-loss-params", default=None, help="HiFi-GAN: fs, fft_size, hop_size, win_length, num_mels, fmin, fmax, log_base; JSON or a yaml file")
    ap.add_argument("--scheduler-milestones", type=_ints, default=None,
                    help="HiFi-GAN: MultiStepLR's milestones, default %s" % ",".join(map(str, HIFIGAN_SCHEDULER["milestones"])))
    ap.add_argument("--verbose", type=int, default=1)
    return ap


CONFIG_KEYS = {"sampling_rate", "hop_size", "generator_type", "generator_params", "discriminator_type", "discriminator_params", "stft_loss_params",
               "lambda_adv", "batch_size", "batch_max_steps", "generator_optimizer_params", "discriminator_optimizer_params", "generator_scheduler_params",
               "discriminator_scheduler_params", "generator_grad_norm", "discriminator_grad_norm", "discriminator_train_start_steps", "train_max_steps",
               "save_interval_steps", "eval_interval_steps", "log_interval_steps", "generator_optimizer_type", "discriminator_optimizer_type",
               "generator_scheduler_type", "discriminator_scheduler_type", "seed"}


def _extras(d, allowed, where):
    """the keys of d outside `allowed`, as `where.key`"""
    return ["%s.%s" % (where, k) if where else str(k) for k in sorted(set(d) - set(allowed), key=str)]


def _refuse(extras):
    if extras:
        raise ValueError("fcl-taco2_amd: train_vocoder: %s not supported: %s" % ("this key is" if len(extras) == 1 else "these keys are", ", ".join(extras)))


def _only(d, allowed, where):
    _refuse(_extras(d, allowed, where))
    return d


def read_config(path):
    """a parallel_wavegan-style config.yml -> the flat values of DEFAULTS' names (plus generator_params / discriminator_params / seed); an unknown or
    unsupported key is refused by name"""
    import yaml

    with open(path) as f:
        y = yaml.safe_load(f) or {}
    # every key that is refused, in one message: a real parallel_wavegan config carries a dozen the driver has no use for
    bad = _extras(y, CONFIG_KEYS, "")
    for sec, allowed in (("generator_params", GENERATOR_DEFAULTS), ("discriminator_params", DISCRIMINATOR_DEFAULTS),
                         ("stft_loss_params", ("fft_sizes", "hop_sizes", "win_lengths")), ("generator_optimizer_params", ("lr", "eps")),
                         ("discriminator_optimizer_params", ("lr", "eps")), ("generator_scheduler_params", ("step_size", "gamma")),
                         ("discriminator_scheduler_params", ("step_size", "gamma"))):
        if isinstance(y.get(sec), dict):
            bad += _extras(y[sec], allowed, sec)
    _refuse(bad)
    for k, want in (("generator_type", "ParallelWaveGANGenerator"), ("discriminator_type", "ParallelWaveGANDiscriminator"), ("generator_optimizer_type", "RAdam"),
                    ("discriminator_optimizer_type", "RAdam"), ("generator_scheduler_type", "StepLR"), ("discriminator_scheduler_type", "StepLR")):
        if y.get(k, want) != want:
            raise ValueError("fcl-taco2_amd: train_vocoder: config key %s=%r is not supported (%s)" % (k, y[k], want))
    out = {k: y[k] for k in ("sampling_rate", "hop_size", "generator_params", "discriminator_params", "lambda_adv", "batch_size", "batch_max_steps",
                             "generator_grad_norm", "discriminator_grad_norm", "discriminator_train_start_steps", "train_max_steps", "save_interval_steps",
                             "eval_interval_steps", "log_interval_steps", "seed") if k in y}
    for k in ("fft_sizes", "hop_sizes", "win_lengths"):
        if k in _only(y.get("stft_loss_params", {}), ("fft_sizes", "hop_sizes", "win_lengths"), "stft_loss_params"):
            out[k] = tuple(y["stft_loss_params"][k])
    lr = {"generator": {}, "discriminator": {}}
    for net in lr:
        o = _only(y.get(net + "_optimizer_params", {}), ("lr", "eps"), net + "_optimizer_params")
        s = _only(y.get(net + "_scheduler_params", {}), ("step_size", "gamma"), net + "_scheduler_params")
        if "lr" in o:
            out[net + "_lr"] = float(o["lr"])
        lr[net] = (o.get("eps"), s.get("step_size"), s.get("gamma"))
    for i, k in enumerate(("optimizer_eps", "scheduler_step_size", "scheduler_gamma")):
        a, b = lr["generator"][i], lr["discriminator"][i]
        if a is not None and b is not None and a != b:
            raise ValueError("fcl-taco2_amd: train_vocoder: config key %s differs between the two networks (%r, %r): one value serves both" % (k, a, b))
        if a is not None or b is not None:
            out[k] = a if a is not None else b
    return out


# flags that belong to one recipe and are refused under the other
PWG_ONLY_FLAGS = ("ends", "scheduler_step_size", "optimizer_eps", "fft_sizes", "hop_sizes", "win_lengths")
HIFIGAN_ONLY_FLAGS = ("output_end", "lambda_aux", "lambda_feat_match", "mel_loss_params", "scheduler_milestones")


def recipe_of(args):
    """the generator_type that selects the recipe: the flag, else the key of --config, else Parallel WaveGAN"""
    gtype = getattr(args, "generator_type", None)
    if gtype is None and args.config:
        import yaml

        with open(args.config) as f:
            gtype = (yaml.safe_load(f) or {}).get("generator_type")
    gtype = PWG_TYPE if gtype is None else gtype
    if gtype not in (PWG_TYPE, HIFIGAN_TYPE):
        raise ValueError("fcl-taco2_amd: train_vocoder: generator_type=%r is not supported (%s, %s)" % (gtype, PWG_TYPE, HIFIGAN_TYPE))
    return gtype


def _refuse_flags(args, names, recipe):
    given = ["--" + k.replace("_", "-") for k in names if getattr(args, k, None) is not None]
    if given:
        raise ValueError("fcl-taco2_amd: train_vocoder: %s %s not a flag of the %s recipe" % (", ".join(given), "is" if len(given) == 1 else "are", recipe))


def log_base_factor(log_base):
    """what the mel loss's scalar (an L1 of log10 mels) is multiplied by under mel_loss_params.log_base: |log_b x - log_b y| = (ln 10 / ln b) |log10 x -
    log10 y| exactly; null is the natural logarithm"""
    if log_base is None:
        return math.log(10.0)
    if not (isinstance(log_base, (int, float)) and log_base > 0 and log_base != 1):
        raise ValueError("fcl-taco2_amd: train_vocoder: mel_loss_params.log_base=%r is not a base (null: natural, or a positive number other than 1)" % (log_base,))
    return 1.0 if float(log_base) == 10.0 else math.log(10.0) / math.log(float(log_base))


HIFIGAN_CONFIG_KEYS = {"sampling_rate", "hop_size", "generator_type", "generator_params", "discriminator_type", "discriminator_params", "mel_loss_params",
                       "lambda_aux", "lambda_adv", "lambda_feat_match", "batch_size", "batch_max_steps", "generator_optimizer_type",
                       "generator_optimizer_params", "generator_scheduler_type", "generator_scheduler_params", "generator_grad_norm",
                       "discriminator_optimizer_type", "discriminator_optimizer_params", "discriminator_scheduler_type", "discriminator_scheduler_params",
                       "discriminator_grad_norm", "generator_train_start_steps", "discriminator_train_start_steps", "train_max_steps", "save_interval_steps",
                       "eval_interval_steps", "log_interval_steps", "seed"}
HIFIGAN_SECTIONS = (("generator_params", HIFIGAN_GENERATOR_DEFAULTS), ("discriminator_params", HIFIGAN_DISCRIMINATOR_DEFAULTS), ("mel_loss_params", HIFIGAN_MEL_LOSS),
                    ("generator_optimizer_params", HIFIGAN_OPTIMIZER), ("discriminator_optimizer_params", HIFIGAN_OPTIMIZER),
                    ("generator_scheduler_params", HIFIGAN_SCHEDULER), ("discriminator_scheduler_params", HIFIGAN_SCHEDULER))


def resolve_hifigan(args):
    """resolve() under the HiFi-GAN recipe: its own table of defaults and of allowed keys, the same layout"""
    from . import hifigan, hifigan_generator, mel_loss

    _refuse_flags(args, PWG_ONLY_FLAGS, "HiFi-GAN")
    file = {}
    if args.config:
        import yaml

        with open(args.config) as f:
            file = yaml.safe_load(f) or {}
    bad = _extras(file, HIFIGAN_CONFIG_KEYS, "")
    for sec, allowed in HIFIGAN_SECTIONS:
        if isinstance(file.get(sec), dict):
            bad += _extras(file[sec], allowed, sec)
    dfile = file.get("discriminator_params") if isinstance(file.get("discriminator_params"), dict) else {}
    for sec, allowed in (("scale_discriminator_params", HIFIGAN_SCALE_DEFAULTS), ("period_discriminator_params", HIFIGAN_PERIOD_DEFAULTS)):
        if isinstance(dfile.get(sec), dict):
            bad += _extras(dfile[sec], allowed, "discriminator_params." + sec)
    _refuse(bad)
    for k, want in (("discriminator_type", HIFIGAN_DISCRIMINATOR), ("generator_optimizer_type", "Adam"), ("discriminator_optimizer_type", "Adam"),
                    ("generator_scheduler_type", "MultiStepLR"), ("discriminator_scheduler_type", "MultiStepLR")):
        if file.get(k, want) != want:
            raise ValueError("fcl-taco2_amd: train_vocoder: config key %s=%r is not supported (%s)" % (k, file[k], want))
    base = dict(HIFIGAN_DEFAULTS, seed=0)
    base.update({k: v for k, v in file.items() if k in base})
    for k in base:
        if getattr(args, k, None) is not None:
            base[k] = getattr(args, k)
    if int(base["generator_train_start_steps"]) != 1:
        raise ValueError("fcl-taco2_amd: train_vocoder: generator_train_start_steps=%r is not supported (1: the generator trains from the first step)"
                         % (base["generator_train_start_steps"],))
    gp = dict(HIFIGAN_GENERATOR_DEFAULTS, **file.get("generator_params", {}))
    gp.update(_params(args.generator_params, "--generator-params"))
    _only(gp, HIFIGAN_GENERATOR_DEFAULTS, "generator_params")
    hifigan_generator.check_training(hifigan.config({k: v for k, v in gp.items() if k in hifigan.CONFIG}))
    dp = dict(HIFIGAN_DISCRIMINATOR_DEFAULTS, **dfile)
    dp.update(_params(args.discriminator_params, "--discriminator-params"))
    _only(dp, HIFIGAN_DISCRIMINATOR_DEFAULTS, "discriminator_params")
    for sec, dflt in (("scale_discriminator_params", HIFIGAN_SCALE_DEFAULTS), ("period_discriminator_params", HIFIGAN_PERIOD_DEFAULTS)):
        dp[sec] = dict(dflt, **_only(dict(dp[sec] or {}), dflt, "discriminator_params." + sec))
    fs = int(base["sampling_rate"])
    mp = dict(HIFIGAN_MEL_LOSS, fs=fs)
    mp.update(file.get("mel_loss_params") or {})
    mp.update(_params(args.mel_loss_params, "--mel-loss-params"))
    _only(mp, HIFIGAN_MEL_LOSS, "mel_loss_params")
    if mp["fmax"] is None:
        mp["fmax"] = mp["fs"] / 2
    log_base_factor(mp["log_base"])
    mel_loss.check_configuration(mp["fs"], [mp["fft_size"]], [mp["hop_size"]], [mp["win_length"]], mp["num_mels"], mp["fmin"], mp["fmax"])
    hop = int(np.prod(gp["upsample_scales"]))
    if "hop_size" in file and int(file["hop_size"]) != hop:
        raise ValueError("fcl-taco2_amd: train_vocoder: config key hop_size=%r is not the product of upsample_scales (%d)" % (file["hop_size"], hop))
    if base["batch_max_steps"] % hop or base["batch_max_steps"] < hop:
        raise ValueError("fcl-taco2_amd: train_vocoder: batch_max_steps=%d is not a positive multiple of the hop (%d)" % (base["batch_max_steps"], hop))
    for k in ("batch_size", "train_max_steps", "save_interval_steps", "eval_interval_steps", "log_interval_steps"):
        if int(base[k]) < 1:
            raise ValueError("fcl-taco2_amd: train_vocoder: %s=%r must be positive" % (k, base[k]))
    if int(base["discriminator_train_start_steps"]) < 0:
        raise ValueError("fcl-taco2_amd: train_vocoder: discriminator_train_start_steps=%r must not be negative" % (base["discriminator_train_start_steps"],))
    out = {"sampling_rate": fs, "hop_size": hop, "generator_type": HIFIGAN_TYPE, "generator_params": gp, "discriminator_type": HIFIGAN_DISCRIMINATOR,
           "discriminator_params": dp, "mel_loss_params": mp, "lambda_aux": float(base["lambda_aux"]), "lambda_adv": float(base["lambda_adv"]),
           "lambda_feat_match": float(base["lambda_feat_match"]), "batch_size": int(base["batch_size"]), "batch_max_steps": int(base["batch_max_steps"])}
    for net in ("generator", "discriminator"):
        o = dict(HIFIGAN_OPTIMIZER, **(file.get(net + "_optimizer_params") or {}))
        if getattr(args, net + "_lr", None) is not None:
            o["lr"] = getattr(args, net + "_lr")
        sc = dict(HIFIGAN_SCHEDULER, **(file.get(net + "_scheduler_params") or {}))
        if args.scheduler_gamma is not None:
            sc["gamma"] = args.scheduler_gamma
        if args.scheduler_milestones is not None:
            sc["milestones"] = list(args.scheduler_milestones)
        ms = [int(m) for m in sc["milestones"]]
        if ms != sorted(ms) or (ms and ms[0] < 1):
            raise ValueError("fcl-taco2_amd: train_vocoder: %s_scheduler_params.milestones=%r must be ascending positive steps" % (net, sc["milestones"]))
        out[net + "_optimizer_type"] = "Adam"
        out[net + "_optimizer_params"] = {"lr": float(o["lr"]), "betas": [float(b) for b in o["betas"]], "weight_decay": float(o["weight_decay"])}
        out[net + "_scheduler_type"] = "MultiStepLR"
        out[net + "_scheduler_params"] = {"gamma": float(sc["gamma"]), "milestones": ms}
        out[net + "_grad_norm"] = float(base[net + "_grad_norm"])
    out.update({k: int(base[k]) for k in ("generator_train_start_steps", "discriminator_train_start_steps", "train_max_steps", "save_interval_steps",
                                          "eval_interval_steps", "log_interval_steps", "seed")})
    return json.loads(json.dumps(out))  # (plain containers: what config.yml holds)


def resolve(args):
    """flags over --config over the selected recipe's defaults -> the run's config in parallel_wavegan's layout (what config.yml holds)"""
    from . import pwg_discriminator, pwg_generator, stft_loss

    if recipe_of(args) == HIFIGAN_TYPE:
        return resolve_hifigan(args)
    _refuse_flags(args, HIFIGAN_ONLY_FLAGS, "Parallel WaveGAN")
    base = dict(DEFAULTS, seed=0)
    file = read_config(args.config) if args.config else {}
    base.update({k: v for k, v in file.items() if k in base})
    for k in base:
        if getattr(args, k, None) is not None:
            base[k] = getattr(args, k)
    gp = dict(GENERATOR_DEFAULTS, **file.get("generator_params", {}))
    gp.update(_params(args.generator_params, "--generator-params"))
    dp = dict(DISCRIMINATOR_DEFAULTS, **file.get("discriminator_params", {}))
    dp.update(_params(args.discriminator_params, "--discriminator-params"))
    _only(gp, GENERATOR_DEFAULTS, "generator_params")
    _only(dp, DISCRIMINATOR_DEFAULTS, "discriminator_params")
    gp["upsample_params"] = {"upsample_scales": [int(s) for s in _only(dict(gp["upsample_params"]), ("upsample_scales",), "upsample_params")["upsample_scales"]]}
    pwg_generator.check_configuration(**gp)
    pwg_generator.check_ends(gp["upsample_params"]["upsample_scales"], gp["aux_context_window"])
    slope = dict(dp["nonlinear_activation_params"] or {})
    _only(slope, ("negative_slope",), "nonlinear_activation_params")
    pwg_discriminator.check_configuration(**dict({k: v for k, v in dp.items() if k != "nonlinear_activation_params"}, **slope))
    stft_loss.check_resolutions(base["fft_sizes"], base["hop_sizes"], base["win_lengths"])
    hop = int(np.prod(gp["upsample_params"]["upsample_scales"]))
    if "hop_size" in file and int(file["hop_size"]) != hop:
        raise ValueError("fcl-taco2_amd: train_vocoder: config key hop_size=%r is not the product of upsample_scales (%d)" % (file["hop_size"], hop))
    if base["batch_max_steps"] % hop or base["batch_max_steps"] < hop:
        raise ValueError("fcl-taco2_amd: train_vocoder: batch_max_steps=%d is not a positive multiple of the hop (%d)" % (base["batch_max_steps"], hop))
    for k in ("batch_size", "train_max_steps", "save_interval_steps", "eval_interval_steps", "log_interval_steps", "scheduler_step_size"):
        if int(base[k]) < 1:
            raise ValueError("fcl-taco2_amd: train_vocoder: %s=%r must be positive" % (k, base[k]))
    opt = lambda net: {"lr": float(base[net + "_lr"]), "eps": float(base["optimizer_eps"])}
    sch = {"step_size": int(base["scheduler_step_size"]), "gamma": float(base["scheduler_gamma"])}
    return {"sampling_rate": int(base["sampling_rate"]), "hop_size": hop, "generator_type": "ParallelWaveGANGenerator", "generator_params": gp,
            "discriminator_type": "ParallelWaveGANDiscriminator", "discriminator_params": dp,
            "stft_loss_params": {k: [int(v) for v in base[k]] for k in ("fft_sizes", "hop_sizes", "win_lengths")}, "lambda_adv": float(base["lambda_adv"]),
            "batch_size": int(base["batch_size"]), "batch_max_steps": int(base["batch_max_steps"]), "generator_optimizer_type": "RAdam",
            "generator_optimizer_params": opt("generator"), "generator_scheduler_type": "StepLR", "generator_scheduler_params": dict(sch),
            "generator_grad_norm": float(base["generator_grad_norm"]), "discriminator_optimizer_type": "RAdam",
            "discriminator_optimizer_params": opt("discriminator"), "discriminator_scheduler_type": "StepLR", "discriminator_scheduler_params": dict(sch),
            "discriminator_grad_norm": float(base["discriminator_grad_norm"]),
            "discriminator_train_start_steps": int(base["discriminator_train_start_steps"]), "train_max_steps": int(base["train_max_steps"]),
            "save_interval_steps": int(base["save_interval_steps"]), "eval_interval_steps": int(base["eval_interval_steps"]),
            "log_interval_steps": int(base["log_interval_steps"]), "seed": int(base["seed"])}


def adversarial(cfg, step):
    """whether step `step` (1-based) has an adversarial term and a discriminator update: the first is discriminator_train_start_steps + 1 (0: every step)"""
    return step > cfg["discriminator_train_start_steps"]


def learning_rate(cfg, net, step):
    """the learning rate step `step` (1-based) is taken with: StepLR, or MultiStepLR (the milestones passed), after step - 1 scheduler steps"""
    s = cfg[net + "_scheduler_params"]
    if "milestones" in s:
        return cfg[net + "_optimizer_params"]["lr"] * s["gamma"] ** sum(1 for m in s["milestones"] if step - 1 >= m)
    return cfg[net + "_optimizer_params"]["lr"] * s["gamma"] ** ((step - 1) // s["step_size"])


class Windows(object):
    """the window sampler (parallel_wavegan's collater): an utterance of T mel frames gives windows of `frames` frames starting at f0 in
    [ctx, T - ctx - frames], the mel rows [f0 - ctx, f0 + frames + ctx) and the samples [f0 hop, (f0 + frames) hop).  batch(step) is a function of
    (seed, step) alone: utterances from a permutation per epoch, window starts and noise from generators seeded by (seed, stream, step)."""

    def __init__(self, lengths, frames, ctx, hop, batch_size, seed):
        """lengths: [(utt id, mel frames)]"""
        self.frames, self.ctx, self.hop, self.batch_size, self.seed = int(frames), int(ctx), int(hop), int(batch_size), int(seed)
        self.utts = [(u, int(T)) for u, T in lengths if int(T) - 2 * self.ctx - self.frames >= 0]
        self.dropped = [u for u, T in lengths if int(T) - 2 * self.ctx - self.frames < 0]
        if not self.utts:
            raise ValueError("fcl-taco2_amd: train_vocoder: no utterance is long enough for one window of %d frames + 2 x %d of context (%d given: %s)"
                             % (self.frames, self.ctx, len(lengths), ", ".join(self.dropped[:10])))

    def _rng(self, stream, n):
        return np.random.default_rng([self.seed, stream, n])

    def epoch(self, step):
        """the epochs finished before step `step`'s last item"""
        return (step * self.batch_size - 1) // len(self.utts)

    def batch(self, step):
        """-> [(utt index, f0)] of step `step` (1-based)"""
        n, out = len(self.utts), []
        starts = self._rng(2, step).random(self.batch_size)
        for i in range(self.batch_size):
            p = (step - 1) * self.batch_size + i
            k = int(self._rng(1, p // n).permutation(n)[p % n])
            lo, hi = self.ctx, self.utts[k][1] - self.ctx - self.frames
            out.append((k, lo + min(int(starts[i] * (hi - lo + 1)), hi - lo)))
        return out

    def noise(self, step):
        return self._rng(3, step).standard_normal((self.batch_size, 1, self.frames * self.hop), dtype=np.float32)

    def valid(self, k):
        """the one fixed window and noise of validation utterance k"""
        lo, hi = self.ctx, self.utts[k][1] - self.ctx - self.frames
        return lo + min(int(self._rng(4, k).random() * (hi - lo + 1)), hi - lo), self._rng(5, k).standard_normal((1, 1, self.frames * self.hop), dtype=np.float32)

    def cut(self, mel, wav, f0):
        """-> (mel window [frames + 2 ctx, n_mels], wav window [frames hop])"""
        return mel[f0 - self.ctx : f0 + self.frames + self.ctx], wav[f0 * self.hop : (f0 + self.frames) * self.hop]


class Corpus(object):
    """mels/<utt>.npy and the wavs of a list of ids; lengths from the headers, T = samples // hop + 1 checked by id before the first device call"""

    def __init__(self, ids, wavs, feature_root, fs, hop, n_mels):
        self.fs, self.paths = fs, []
        for u in ids:
            if u not in wavs:
                raise ValueError("%s: no wav for this utterance id" % u)
            mp = os.path.join(feature_root, "mels", u + ".npy")
            if not os.path.exists(mp):
                raise ValueError("%s: %s does not exist" % (u, mp))
            m = np.load(mp, mmap_mode="r")
            L = XF.wav_samples(wavs[u], fs)
            if m.ndim != 2 or m.shape[1] != n_mels or m.shape[0] != L // hop + 1:
                raise ValueError("%s: a [%d, %d] mel expected for %d samples at hop %d, got %r" % (u, L // hop + 1, n_mels, L, hop, tuple(m.shape)))
            self.paths.append((u, mp, wavs[u], int(m.shape[0])))
        self.by_id = {p[0]: p for p in self.paths}

    def lengths(self):
        return [(u, T) for u, _, _, T in self.paths]

    def load(self, u):
        _, mp, wp, _ = self.by_id[u]
        return np.load(mp).astype(np.float32), XF.read_wav(wp, self.fs)


def checkpoint_of(gen, disc, opt, sch, steps, epochs):
    return {"model": {"generator": gen.state_dict(), "discriminator": disc.state_dict()},
            "optimizer": {"generator": opt["generator"].state_dict(), "discriminator": opt["discriminator"].state_dict()},
            "scheduler": {"generator": sch["generator"].state_dict(), "discriminator": sch["discriminator"].state_dict()}, "steps": int(steps),
            "epochs": int(epochs)}


def check_resume(cfg, path):
    """the config.yml beside a checkpoint against this run's values: a disagreement on a model or optimiser value is refused naming the key"""
    import yaml

    side = os.path.join(os.path.dirname(os.path.abspath(path)), "config.yml")
    if not os.path.exists(side):
        raise ValueError("fcl-taco2_amd: train_vocoder: --resume %s has no config.yml beside it" % path)
    with open(side) as f:
        old = yaml.safe_load(f) or {}
    for k in PINNED:
        if old.get(k) != json.loads(json.dumps(cfg.get(k))):
            raise ValueError("fcl-taco2_amd: train_vocoder: --resume: %s is %r in %s and %r now" % (k, old.get(k), side, cfg.get(k)))


def _read_ids(path):
    with open(path) as f:
        return [ln.split()[0] for ln in f if ln.strip()]


class Trainer(object):
    dp = None  # a vocoder_dp.DataParallel under a process group (main attaches it); None: one process, and the step is the one-GPU step as it was

    def _zero(self, net):
        """before a backward pass of `net`: no gradients, or under data parallelism a zeroed arena with its hooks armed"""
        if self.dp is None:
            self.opt[net].zero_grad()
        else:
            self.dp.begin(net)

    def _exchange(self, net):
        """after that backward pass: every rank's gradient of `net` becomes the rank mean"""
        if self.dp is not None:
            self.dp.finish(net)

    def _agree(self, out):
        """the phase's logged scalars as every rank will see them: the rank means, in one collective"""
        return out if self.dp is None else self.dp.mean_terms(out)

    def __init__(self, cfg, device, ends="hip"):
        from .pwg_discriminator import ParallelWaveGANDiscriminator
        from .pwg_generator import TrainableParallelWaveGANGenerator
        from .stft_loss import MultiResolutionSTFTLoss

        self.cfg, self.dev, self.ends = cfg, device, ends
        torch.manual_seed(cfg["seed"])  # (the initial weights)
        self.gen = TrainableParallelWaveGANGenerator(**cfg["generator_params"]).to(device)
        self.disc = ParallelWaveGANDiscriminator(**cfg["discriminator_params"]).to(device)
        s = cfg["stft_loss_params"]
        self.criterion = MultiResolutionSTFTLoss(device, tuple(s["fft_sizes"]), tuple(s["hop_sizes"]), tuple(s["win_lengths"]))
        nets = {"generator": self.gen, "discriminator": self.disc}
        self.opt = {k: torch.optim.RAdam(n.parameters(), **cfg[k + "_optimizer_params"]) for k, n in nets.items()}
        self.sch = {k: torch.optim.lr_scheduler.StepLR(self.opt[k], **cfg[k + "_scheduler_params"]) for k in nets}
        self.steps = 0

    def load(self, path, models_only=False):
        ck = torch.load(path, map_location=self.dev, weights_only=True)
        self.gen.load_state_dict(ck["model"]["generator"])
        self.disc.load_state_dict(ck["model"]["discriminator"])
        if not models_only:
            for k in self.opt:
                self.opt[k].load_state_dict(ck["optimizer"][k])
                self.sch[k].load_state_dict(ck["scheduler"][k])
            self.steps = int(ck["steps"])

    def _finite(self, step, **terms):
        for k, v in terms.items():
            if not math.isfinite(v):
                raise FloatingPointError("fcl-taco2_amd: train_vocoder: step %d: %s is %r; no checkpoint of this step is written" % (step, k, v))

    def losses(self, z, c, wav, adv):
        """the generator's terms on one batch (the graph attached) -> (fake, {term: tensor})"""
        from .pwg_discriminator import generator_adversarial_loss

        fake = self.gen(z, c, ends=self.ends)
        sc, mag = self.criterion(fake, wav)
        terms = {"spectral_convergence_loss": sc, "log_stft_magnitude_loss": mag}
        if adv:
            # No discriminator weight gradient is computed in the generator's backward pass.  The parameters may be released again BEFORE backward():
            # the discriminator's autograd function decides at forward time which gradients it owes (needs_input_grad), and its folded weights were
            # formed while the parameters were frozen, so nothing on this graph leads to them (tested by the launch record: no pwd_dw* launch).
            for p in self.disc.parameters():
                p.requires_grad_(False)
            terms["adversarial_loss"] = generator_adversarial_loss(self.disc(fake))
            for p in self.disc.parameters():
                p.requires_grad_(True)
        return fake, terms

    def step(self, z, c, wav):
        """one step of parallel_wavegan's trainer -> {term or norm: float}"""
        from .pwg_discriminator import discriminator_adversarial_loss

        cfg, n = self.cfg, self.steps + 1
        adv = adversarial(cfg, n)
        _, terms = self.losses(z, c, wav, adv)
        loss = terms["spectral_convergence_loss"] + terms["log_stft_magnitude_loss"]
        if adv:
            loss = loss + cfg["lambda_adv"] * terms["adversarial_loss"]
        self._zero("generator")
        loss.backward()
        self._exchange("generator")
        out = {k: float(v.detach()) for k, v in terms.items()}
        out["generator_grad_norm"] = float(torch.nn.utils.clip_grad_norm_(self.gen.parameters(), cfg["generator_grad_norm"]))
        out = self._agree(out)
        self._finite(n, **out)
        self.opt["generator"].step()
        self.sch["generator"].step()
        if adv:
            with torch.no_grad():
                fake = self.gen(z, c, ends=self.ends)
            real_loss, fake_loss = discriminator_adversarial_loss(self.disc(wav), self.disc(fake))
            self._zero("discriminator")
            (real_loss + fake_loss).backward()
            self._exchange("discriminator")
            more = dict(real_loss=float(real_loss.detach()), fake_loss=float(fake_loss.detach()))
            more["discriminator_grad_norm"] = float(torch.nn.utils.clip_grad_norm_(self.disc.parameters(), cfg["discriminator_grad_norm"]))
            more = self._agree(more)
            self._finite(n, **more)
            out.update(more)
            self.opt["discriminator"].step()
            self.sch["discriminator"].step()
        self.steps = n
        return out


def feature_matching_loss(feats_fake, feats_real):
    """the recipe's feature matching: the L1 mean of every map but the scores against the detached real map, SUMMED over the layers and over the
    discriminators (average_by_layers and average_by_discriminators both off; hifigan_discriminator.feature_match_loss averages over both)"""
    return sum(torch.mean(torch.abs(f - r.detach())) for fake, real in zip(feats_fake, feats_real) for f, r in zip(fake[:-1], real[:-1]))


class HiFiGANTrainer(Trainer):
    """the hifigan.v1 step in the package trainer's order: the generator on mel (+ adversarial + feature matching once the discriminator is on), its Adam
    and scheduler step, the generator again under no_grad, the discriminator's real / fake loss and its step"""

    LATE = ("adversarial_loss", "feature_matching_loss", "real_loss", "fake_loss", "discriminator_grad_norm")

    def __init__(self, cfg, device, output_end="hip"):
        from .hifigan_generator import TrainableHiFiGANGenerator
        from .hifigan_scale_discriminator import HiFiGANMultiScaleMultiPeriodDiscriminator
        from .mel_loss import MelSpectrogramLoss

        self.cfg, self.dev, self.output_end = cfg, device, output_end
        torch.manual_seed(cfg["seed"])  # (the initial weights)
        self.gen = TrainableHiFiGANGenerator(**cfg["generator_params"]).to(device)
        self.disc = HiFiGANMultiScaleMultiPeriodDiscriminator(**cfg["discriminator_params"]).to(device)
        m = cfg["mel_loss_params"]
        self.criterion = MelSpectrogramLoss(device, m["fs"], (m["fft_size"],), (m["hop_size"],), (m["win_length"],), m["num_mels"], m["fmin"], m["fmax"])
        self.mel_scale = log_base_factor(m["log_base"])
        nets = {"generator": self.gen, "discriminator": self.disc}
        adam = lambda p: dict(lr=p["lr"], betas=tuple(p["betas"]), weight_decay=p["weight_decay"])
        self.opt = {k: torch.optim.Adam(n.parameters(), **adam(cfg[k + "_optimizer_params"])) for k, n in nets.items()}
        self.sch = {k: torch.optim.lr_scheduler.MultiStepLR(self.opt[k], **cfg[k + "_scheduler_params"]) for k in nets}
        self.steps = 0

    def losses(self, c, wav, adv):
        """the generator's terms on one batch (the graph attached) -> (fake, {term: tensor})"""
        from .hifigan_discriminator import generator_adversarial_loss, split_batch

        fake = self.gen(c, output_end=self.output_end)
        terms = {"mel_loss": self.mel_scale * self.criterion(fake, wav)}
        if adv:
            # as Trainer.losses: the discriminator is frozen around its forward, so the generator's backward launches none of its weight gradients; real and
            # fake go through it packed into one forward (the two halves have the same lengths) and are split again
            for p in self.disc.parameters():
                p.requires_grad_(False)
            outs_real, outs_fake = split_batch(self.disc(torch.cat([wav[:, 0], fake[:, 0]])))
            for p in self.disc.parameters():
                p.requires_grad_(True)
            terms["adversarial_loss"] = generator_adversarial_loss(outs_fake)
            terms["feature_matching_loss"] = feature_matching_loss(outs_fake, outs_real)
        return fake, terms

    def _norm(self, params, limit):
        """the gradient norm, clipped to `limit` when that is positive"""
        return float(torch.nn.utils.clip_grad_norm_(params, limit if limit > 0 else float("inf")))

    def step(self, c, wav):
        from .hifigan_discriminator import discriminator_adversarial_loss

        cfg, n = self.cfg, self.steps + 1
        adv = adversarial(cfg, n)
        _, terms = self.losses(c, wav, adv)
        loss = cfg["lambda_aux"] * terms["mel_loss"]
        if adv:
            loss = loss + cfg["lambda_adv"] * terms["adversarial_loss"] + cfg["lambda_feat_match"] * terms["feature_matching_loss"]
        self._zero("generator")
        loss.backward()
        self._exchange("generator")
        out = {k: float(v.detach()) for k, v in terms.items()}
        out["generator_grad_norm"] = self._norm(self.gen.parameters(), cfg["generator_grad_norm"])
        out = self._agree(out)
        self._finite(n, **out)
        self.opt["generator"].step()
        self.sch["generator"].step()
        if adv:
            with torch.no_grad():
                fake = self.gen(c, output_end=self.output_end)
            real_loss, fake_loss = discriminator_adversarial_loss(self.disc(wav), self.disc(fake))
            self._zero("discriminator")
            (real_loss + fake_loss).backward()
            self._exchange("discriminator")
            more = dict(real_loss=float(real_loss.detach()), fake_loss=float(fake_loss.detach()))
            more["discriminator_grad_norm"] = self._norm(self.disc.parameters(), cfg["discriminator_grad_norm"])
            more = self._agree(more)
            self._finite(n, **more)
            out.update(more)
            self.opt["discriminator"].step()
            self.sch["discriminator"].step()
        self.steps = n
        return out


def shard(items, rank, world):
    """rank's share of a global batch (or of its noise rows, or of the validation windows): the items i with i % world == rank, in order"""
    return items[rank::world]


def check_gpus(n):
    if not 1 <= int(n) <= MAX_RANKS:
        raise ValueError("fcl-taco2_amd: train_vocoder: --gpus %d is not supported: 1 to %d ranks on one node" % (n, MAX_RANKS))


def check_ranks(world, backend, devices):
    """RCCL takes one GPU per rank; refused before the first device call"""
    if backend == "nccl" and world > devices:
        raise ValueError("fcl-taco2_amd: train_vocoder: --dist-backend nccl: %d ranks but %d GPU%s; RCCL takes one GPU per rank (gloo lets ranks share one)"
                         % (world, devices, "" if devices == 1 else "s"))


def check_batch(batch_size, world):
    """batch_size is the GLOBAL batch: every rank takes batch_size / world items of it"""
    if batch_size % world:
        raise ValueError("fcl-taco2_amd: train_vocoder: batch_size=%d is not a multiple of the %d ranks (batch_size is the global batch; parallel_wavegan's "
                         "is per process)" % (batch_size, world))


def _free_port():
    import socket

    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    return port


def self_launch(gpus, argv):
    """--gpus N without a torch.distributed environment: start the N ranks as children of torch.distributed.run (one node, rendezvous on 127.0.0.1), as
    bench.py does, and pass their exit code through.  This process makes no device call."""
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # (where `import fcl_taco2_amd` resolves)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(gpus), "--master-addr", "127.0.0.1", "--master-port",
           str(_free_port()), "-m", "fcl_taco2_amd.train_vocoder"] + list(argv)
    path = os.pathsep.join(p for p in (root, os.environ.get("PYTHONPATH")) if p)
    env = dict(os.environ, PYTHONPATH=path, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return subprocess.run(cmd, env=env).returncode


def init_group(backend, rank, world, timeout, device=None):
    """join the job's process group with a finite timeout: a rank that has died ends the job instead of hanging it"""
    import datetime

    import torch.distributed as dist

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if "MASTER_PORT" not in os.environ:
        if world > 1:
            raise ValueError("fcl-taco2_amd: train_vocoder: WORLD_SIZE=%d without MASTER_PORT" % world)
        os.environ["MASTER_PORT"] = str(_free_port())
    more = {"device_id": device} if backend == "nccl" and device is not None else {}
    dist.init_process_group(backend, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=timeout), **more)
    return dist


def dry_run_launch(rank, world, timeout):
    """--dry-run-launch: the launch path alone -- every rank joins over gloo and contributes a one to one all-reduce; rank 0 prints the JSON line"""
    dist = init_group("gloo", rank, world, timeout) if world > 1 else None
    ones = torch.ones(1, dtype=torch.float64)
    if dist is not None:
        dist.all_reduce(ones)
    if rank == 0:
        print(json.dumps({"metric": "dry run of the launcher (no GPU work)", "dry_run": True, "n_gpus": world, "sum_of_ones": float(ones)}), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    return 0


def main(argv=None):
    import sys

    ap = build_parser()
    args = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO if args.verbose else logging.WARN, format="%(asctime)s %(levelname)s: %(message)s")
    check_gpus(args.gpus)
    launched = "WORLD_SIZE" in os.environ  # under torch.distributed.run (or a test's own environment): this process is one rank
    if args.gpus > 1 and not launched:
        return self_launch(args.gpus, sys.argv[1:] if argv is None else argv)
    rank, world, local_rank = (int(os.environ.get(k, d)) for k, d in (("RANK", "0"), ("WORLD_SIZE", "1"), ("LOCAL_RANK", "0")))
    check_gpus(world)
    if args.gpus > 1 and args.gpus != world:
        raise ValueError("fcl-taco2_amd: train_vocoder: --gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    if args.dry_run_launch:
        return dry_run_launch(rank, world, args.dist_timeout)
    # a process group: for more than one rank, and for one rank under GradBuckets' force flag (the N-rank schedule on one card, its collective the
    # identity); without either this is the one-process driver as it was
    grouped = world > 1 or os.environ.get("FCL_DP_FORCE_COLLECTIVE", "0") not in ("", "0")
    if (args.wav_dir is None) == (args.wav_scp is None) or not args.feature_root or not args.train_list or not args.outdir:
        ap.error("--wav-dir or --wav-scp (one of them), --feature-root, --train-list and --outdir are needed")
    if args.resume and args.pretrain:
        ap.error("--resume and --pretrain are exclusive")
    cfg = resolve(args)
    check_batch(cfg["batch_size"], world)
    if grouped:
        check_ranks(world, args.dist_backend, torch.cuda.device_count())  # (counts the devices; initialises none)
    if args.resume:
        check_resume(cfg, args.resume)  # (every rank, before the rendezvous: rank 0 rewrites config.yml only after all have read it)
    try:
        return _train(args, cfg, rank, world, local_rank, grouped)
    finally:
        import torch.distributed as dist

        if grouped and dist.is_initialized():
            dist.destroy_process_group()


def _train(args, cfg, rank, world, local_rank, grouped):
    gp, hifi = cfg["generator_params"], cfg["generator_type"] == HIFIGAN_TYPE
    # (the HiFi-GAN generator takes the window's own frames, no context, and no noise)
    hop, ctx, A, fs = cfg["hop_size"], 0 if hifi else gp["aux_context_window"], gp["in_channels"] if hifi else gp["aux_channels"], cfg["sampling_rate"]
    frames, B = cfg["batch_max_steps"] // hop, cfg["batch_size"]
    mine = B // world  # (this rank's items of the global batch)
    wavs = dict(XF.read_wav_list(args.wav_scp, args.wav_dir))
    train = Corpus(_read_ids(args.train_list), wavs, args.feature_root, fs, hop, A)
    sampler = Windows(train.lengths(), frames, ctx, hop, B, cfg["seed"])
    for u in sampler.dropped:
        logging.warning("%s: too short for one window of %d frames + 2 x %d of context; left out", u, frames, ctx)
    valid = vsampler = None
    if args.valid_list:
        valid = Corpus(_read_ids(args.valid_list), wavs, args.feature_root, fs, hop, A)
        try:
            vsampler = Windows(valid.lengths(), frames, ctx, hop, 1, cfg["seed"])
        except ValueError:
            logging.warning("no validation utterance is long enough for one window: no evaluation lines")
    import yaml

    # ---- the first device call is below (under a process group the rendezvous comes first: every rank has passed the refusals above when it returns)
    dev, dp = torch.device("cuda:0"), None
    if grouped:
        if not torch.cuda.is_available():
            raise RuntimeError("fcl-taco2_amd: train_vocoder: training needs a GPU")
        dev = torch.device("cuda:%d" % (local_rank % torch.cuda.device_count()))
        torch.cuda.set_device(dev)
        init_group(args.dist_backend, rank, world, args.dist_timeout, dev)
    if rank == 0:  # config.yml, train_log.jsonl and the checkpoints are rank 0's alone
        os.makedirs(args.outdir, exist_ok=True)
        with open(os.path.join(args.outdir, "config.yml"), "w") as f:
            yaml.safe_dump(json.loads(json.dumps(cfg)), f, sort_keys=False)
    tr = HiFiGANTrainer(cfg, dev, args.output_end or "hip") if hifi else Trainer(cfg, dev, args.ends or "hip")
    if args.resume:
        tr.load(args.resume)
    elif args.pretrain:
        tr.load(args.pretrain, models_only=True)
    if grouped:
        from .vocoder_dp import DataParallel

        tr.dp = dp = DataParallel(tr)  # (rank 0's parameters and buffers on every rank, the gradient arenas, the hooks)
    log = open(os.path.join(args.outdir, "train_log.jsonl"), "a") if rank == 0 else None
    write = (lambda rec: (log.write(json.dumps(rec) + "\n"), log.flush())) if rank == 0 else (lambda rec: None)
    if sampler.dropped:
        write({"left_out": sampler.dropped})

    def prepare(step):
        """this rank's items of step's batch as pinned host tensors (z, c, wav) -- (c, wav) under the HiFi-GAN recipe -- on the one host thread, while
        the step before it runs; only these windows are loaded"""
        c, w = np.empty((mine, A, frames + 2 * ctx), np.float32), np.empty((mine, 1, frames * hop), np.float32)
        for i, (k, f0) in enumerate(shard(sampler.batch(step), rank, world)):
            mel, wav = train.load(sampler.utts[k][0])
            m, w[i, 0] = sampler.cut(mel, wav, f0)
            c[i] = m.T
        return tuple(torch.from_numpy(a).pin_memory() for a in ((c, w) if hifi else (np.ascontiguousarray(shard(sampler.noise(step), rank, world)), c, w)))

    def evaluate(step):
        sums, n = {}, 0
        if hifi:
            tr.disc.eval()  # (no power iteration of the spectral norm on a validation window)
        with torch.no_grad():
            for k, (u, _) in shard(list(enumerate(vsampler.utts)), rank, world):
                mel, wav = valid.load(u)
                f0, z = vsampler.valid(k)
                m, w = vsampler.cut(mel, wav, f0)
                inputs = (torch.from_numpy(np.ascontiguousarray(m.T[None])).to(dev), torch.from_numpy(np.ascontiguousarray(w[None, None])).to(dev))
                _, terms = tr.losses(*(inputs if hifi else (torch.from_numpy(z).to(dev),) + inputs), adversarial(cfg, step))
                for name, v in terms.items():
                    sums[name] = sums.get(name, 0.0) + float(v)
                n += 1
        if hifi:
            tr.disc.train()
        if dp is not None:  # the ranks' sums and window counts, added in float64 (a rank may have had no window: the names are the step's, not its own)
            adv = adversarial(cfg, step)
            names = ("mel_loss", "adversarial_loss", "feature_matching_loss")[: 3 if adv else 1] if hifi else LOSS_TERMS[: 3 if adv else 2]
            total = dp.sum_float64([sums.get(k, 0.0) for k in names] + [n])
            sums, n = dict(zip(names, total[:-1])), int(total[-1])
        write(dict({"eval_" + k: v / n for k, v in sums.items()}, step=step, eval_windows=n))

    acc, count, t0 = {}, 0, time.perf_counter()
    with concurrent.futures.ThreadPoolExecutor(1) as pool:
        nxt = pool.submit(prepare, tr.steps + 1) if tr.steps < cfg["train_max_steps"] else None
        while tr.steps < cfg["train_max_steps"]:
            n = tr.steps + 1
            batch = [a.to(dev, non_blocking=True) for a in nxt.result()]
            nxt = pool.submit(prepare, n + 1) if n < cfg["train_max_steps"] else None
            lrs = {k: tr.opt[k].param_groups[0]["lr"] for k in tr.opt}
            out = tr.step(*batch)  # (under data parallelism the terms are the rank means, the same floats on every rank)
            for k, v in out.items():
                s, m = acc.get(k, (0.0, 0))
                acc[k] = (s + v, m + 1)
            count += 1
            if n % cfg["log_interval_steps"] == 0:
                torch.cuda.synchronize(dev)
                dt = time.perf_counter() - t0
                rec = dict({k: s / m for k, (s, m) in acc.items()}, step=n, generator_lr=lrs["generator"], discriminator_lr=lrs["discriminator"],
                           ms_per_step=1e3 * dt / count, samples_per_second=count * B * frames * hop / dt)  # (B: the global batch)
                for k in HiFiGANTrainer.LATE if hifi else LOSS_TERMS[2:] + ("discriminator_grad_norm",):
                    rec.setdefault(k, None)  # (before the discriminator starts)
                write(rec)
                logging.info("step %d: %s", n, json.dumps(rec))
                acc, count, t0 = {}, 0, time.perf_counter()
            if vsampler is not None and n % cfg["eval_interval_steps"] == 0:
                evaluate(n)
            if n % cfg["save_interval_steps"] == 0 or n == cfg["train_max_steps"]:
                if dp is not None:  # (raises on every rank, naming the step, if the ranks' networks differ in a bit)
                    dp.same_everywhere("generator", n)
                    dp.same_everywhere("discriminator", n)
                if rank == 0:
                    torch.save(checkpoint_of(tr.gen, tr.disc, tr.opt, tr.sch, n, sampler.epoch(n)), os.path.join(args.outdir, "checkpoint-%dsteps.pkl" % n))
    if rank == 0:
        log.close()
    if dp is not None:
        logging.info("exchange schedule: %s", json.dumps(dp.schedule()))
        import torch.distributed as dist

        dist.barrier()  # (rank 0's last checkpoint is on disk before any rank leaves)
    return tr


if __name__ == "__main__":
    import sys

    done = main()
    sys.exit(done if isinstance(done, int) else 0)  # (the launcher's form returns its ranks' exit code)
