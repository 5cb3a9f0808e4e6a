"""mel -> waveform driver on MI355X: the step the reference delegates to the external `parallel-wavegan-decode --checkpoint vocoder/PWG/PWG.pkl
--feats-scp <decode>/feats.scp --outdir <wav dir>` (inference_student.sh:20-23, inference_teacher.sh:20-23, README.md:46).  Same flag names and
the same outputs (`<outdir>/<utt_id>_gen.wav`, 16-bit PCM at the generator's sampling rate); the generator is selected as that tool selects it, by
`generator_type` of the config.yml: fcl_taco2_amd/vocoder.py (ParallelWaveGANGenerator) or fcl_taco2_amd/hifigan.py (HiFiGANGenerator,
DESIGN.md §6c), both from the published architecture, parity unpinned.  `--griffin-lim` instead of `--checkpoint` needs no trained generator
(fcl_taco2_amd/griffinlim.py): de-normalise with `--mel-stats`, pseudo-inverse mel filterbank, Griffin-Lim; an utterance of T' frames
then gives hop * (T' - 1) samples.

    python -m fcl_taco2_amd.vocoder_decode --checkpoint vocoder/PWG/PWG.pkl --feats-scp exp/student/test/feats.scp --outdir exp/student/test/wav

Utterances are sorted by length and packed into batches of about `--batch-frames` mel frames; batch i + 1 runs on the GPU while batch i's waveform
travels to the host (one packed non-blocking copy on a side stream) and a writer thread encodes the wav files.  `--nj / --job` shard the scp by
utterance (one process per GPU, no collective), like decode.py.
"""
import argparse
import logging
import os
import time
import wave

import numpy as np
import torch

from . import kaldi_io, ops
from .batching import Writer, make_batches  # noqa: F401  (make_batches: also this module's name for it)
from .sharding import shard_utterances
from .vocoder import CONFIG, PWGPlan, ParallelWaveGANGenerator


def generator_config(checkpoint, config=None):
    """Generator geometry from the `config.yml` parallel_wavegan keeps beside its checkpoints (`generator_params`); the v1 defaults without one.
    Returns (cfg overrides for PWGPlan, sampling rate)."""
    return _pwg_config_of(_read_config(checkpoint, config))


def _pwg_config_of(y):
    """generator_config on the parsed config.yml (None: no file)"""
    if y is None:
        return {}, 22050
    gp = y.get("generator_params", {})
    unsupported = {k: gp[k] for k, dflt in (("in_channels", 1), ("out_channels", 1), ("use_causal_conv", False), ("upsample_net", "ConvInUpsampleNetwork"))
                   if gp.get(k, dflt) != dflt}
    if unsupported:  # (dropout is an inference no-op, bias / weight norm are read from the state dict itself)
        raise NotImplementedError("fcl-taco2_amd: generator_params %r are not supported on the HIP path" % unsupported)
    cfg = {k: gp[k] for k in ("layers", "stacks", "residual_channels", "gate_channels", "skip_channels", "aux_channels", "aux_context_window", "kernel_size")
           if k in gp}
    up = gp.get("upsample_params", {})
    bad_up = {k: up[k] for k, dflt in (("nonlinear_activation", None), ("interpolate_mode", "nearest"), ("use_causal_conv", False),
                                       ("freq_axis_kernel_size", 1)) if up.get(k, dflt) != dflt}
    if bad_up:  # they change the upsampling network's arithmetic; silently ignoring them would produce wrong audio
        raise NotImplementedError("fcl-taco2_amd: upsample_params %r are not supported on the HIP path" % bad_up)
    if "upsample_scales" in up:
        cfg["upsample_scales"] = tuple(int(s) for s in up["upsample_scales"])
    return cfg, int(y.get("sampling_rate", 22050))


PWG_TYPE, HIFIGAN_TYPE = "ParallelWaveGANGenerator", "HiFiGANGenerator"


def _read_config(checkpoint, config=None):
    """The parsed config.yml beside the checkpoint (or `config`), None without one."""
    path = config or os.path.join(os.path.dirname(os.path.abspath(checkpoint)), "config.yml")
    if not os.path.exists(path):
        if config:
            raise FileNotFoundError(config)
        return None
    import yaml

    with open(path) as f:
        return yaml.safe_load(f) or {}


def generator_type(checkpoint, config=None):
    """`generator_type` of the config.yml (parallel-wavegan-decode selects the generator class by it); ParallelWaveGANGenerator when the key is
    absent; None without a config.yml (the state-dict keys then decide: family_of_state_dict)."""
    return _type_of(_read_config(checkpoint, config))


def _type_of(y):
    return None if y is None else y.get("generator_type", PWG_TYPE)


def family_of_state_dict(sd):
    """Generator family from the state-dict keys: `input_conv.weight*` is HiFi-GAN's, `first_conv.weight*` Parallel WaveGAN's."""
    if isinstance(sd, dict) and "model" in sd and isinstance(sd["model"], dict) and "generator" in sd["model"]:
        sd = sd["model"]["generator"]
    keys = set(sd)
    if keys & {"input_conv.weight", "input_conv.weight_g", "input_conv.weight_v"}:
        return HIFIGAN_TYPE
    if keys & {"first_conv.weight", "first_conv.weight_g", "first_conv.weight_v"}:
        return PWG_TYPE
    raise NotImplementedError("fcl-taco2_amd: the state dict holds neither input_conv.weight (HiFiGANGenerator) nor first_conv.weight "
                              "(ParallelWaveGANGenerator): unknown generator family")


def hifigan_config(checkpoint, config=None):
    """HiFi-GAN geometry from `generator_params` of the config.yml -> (cfg overrides for HiFiGANPlan, sampling rate).  Parameters the kernels do not
    cover are refused by name (hifigan.config)."""
    return _hifigan_config_of(_read_config(checkpoint, config))


def _hifigan_config_of(y):
    from . import hifigan

    y = y or {}
    gp = dict(y.get("generator_params", {}))
    gp.pop("use_weight_norm", None)  # read from the state dict itself
    unknown = sorted(k for k in gp if k not in hifigan.CONFIG)
    if unknown:
        raise NotImplementedError("fcl-taco2_amd: generator_params %r are not supported on the HIP path" % {k: gp[k] for k in unknown})
    hifigan.config(gp)
    return gp, int(y.get("sampling_rate", 22050))


def hifigan_config_from_shapes(sd):
    """Without a config.yml: channels and kernel sizes from the shapes; what the shapes cannot tell is ASSUMED -- upsampling scale = kernel / 2 and
    dilations (1, 3, 5) per block (as many as the block has convolutions must be 3) -- and logged."""
    if "model" in sd and "generator" in sd["model"]:
        sd = sd["model"]["generator"]
    shape = lambda k: tuple(np.shape(sd[k if k in sd else k + "_v"]))
    has = lambda k: k in sd or k + "_v" in sd
    ch, cin, k = shape("input_conv.weight")
    n = 0
    while has("upsamples.%d.1.weight" % n):
        n += 1
    kus = tuple(shape("upsamples.%d.1.weight" % i)[2] for i in range(n))
    nb = 0
    while has("blocks.%d.convs1.0.1.weight" % nb):
        nb += 1
    if n == 0 or nb == 0 or nb % n:
        raise NotImplementedError("fcl-taco2_amd: cannot read a HiFi-GAN geometry from the state dict (%d upsampling layers, %d blocks)" % (n, nb))
    nk = nb // n
    krs = tuple(shape("blocks.%d.convs1.0.1.weight" % j)[2] for j in range(nk))
    nd = 0
    while has("blocks.0.convs1.%d.1.weight" % nd):
        nd += 1
    if nd != 3 or any(ku % 2 for ku in kus):
        raise NotImplementedError("fcl-taco2_amd: a HiFi-GAN state dict without config.yml is read as scale = kernel / 2 and dilations (1, 3, 5); this one "
                                  "has %d convolutions per block and upsampling kernels %r" % (nd, kus))
    cfg = dict(in_channels=int(cin), out_channels=int(shape("output_conv.1.weight")[0]), channels=int(ch), kernel_size=int(k),
               upsample_scales=tuple(ku // 2 for ku in kus), upsample_kernel_sizes=kus, resblock_kernel_sizes=krs, resblock_dilations=((1, 3, 5),) * nk)
    logging.warning("no config.yml beside the HiFi-GAN checkpoint: ASSUMING upsample_scales %r (= kernel / 2) and resblock_dilations (1, 3, 5); channels %d, "
                    "kernel sizes %r / %r are read from the shapes", cfg["upsample_scales"], ch, kus, krs)
    return cfg, 22050


def build_generator(checkpoint, device, config=None, allow_pickle=False):
    """Generator of a checkpoint + its sampling rate, by `generator_type` of the config.yml (absent / ParallelWaveGANGenerator: vocoder.py;
    HiFiGANGenerator: hifigan.py; anything else: NotImplementedError naming it) or, without a config.yml, by the state-dict keys."""
    y = _read_config(checkpoint, config)  # read once: the type and the geometry come from the same parse
    gtype = _type_of(y)
    if gtype is not None and gtype not in (PWG_TYPE, HIFIGAN_TYPE):
        raise NotImplementedError("fcl-taco2_amd: generator_type %r is not supported on the HIP path (%s and %s are)" % (gtype, PWG_TYPE, HIFIGAN_TYPE))
    sd = load_checkpoint(checkpoint, allow_pickle)
    from_keys = gtype is None
    if from_keys:
        gtype = family_of_state_dict(sd)
    if gtype == HIFIGAN_TYPE:
        from .hifigan import HiFiGANGenerator, HiFiGANPlan

        cfg, rate = hifigan_config_from_shapes(sd) if from_keys else _hifigan_config_of(y)
        return HiFiGANGenerator(HiFiGANPlan(sd, device, cfg)), rate
    cfg, rate = _pwg_config_of(y)
    return ParallelWaveGANGenerator(PWGPlan(sd, device, cfg)), rate


def load_checkpoint(path, allow_pickle=False):
    """torch.load of a parallel_wavegan checkpoint ({"model": {"generator": sd}}, or a bare state dict) -> the same nesting with numpy arrays.
    Loaded with weights_only=True (tensors and plain containers only); a checkpoint that needs the full unpickler — which executes whatever code
    the file carries — is read only with allow_pickle=True (`--unsafe-pickle`), i.e. when the caller vouches for the file."""
    def conv(o):
        if torch.is_tensor(o):
            return o.detach().cpu().float().numpy()
        if isinstance(o, dict):
            return {k: conv(v) for k, v in o.items()}
        return o

    try:
        obj = torch.load(path, map_location="cpu", weights_only=True)
    except Exception as e:
        if not allow_pickle:
            raise RuntimeError("fcl-taco2_amd: %s does not load with weights_only=True (%s); pass --unsafe-pickle / allow_pickle=True only for a "
                               "checkpoint you trust" % (path, str(e).splitlines()[0] if str(e) else type(e).__name__))
        obj = torch.load(path, map_location="cpu", weights_only=False)
    if isinstance(obj, dict) and "model" in obj and isinstance(obj["model"], dict) and "generator" in obj["model"]:
        return {"model": {"generator": conv(obj["model"]["generator"])}}  # (the discriminator / optimizer states are not needed)
    return conv(obj)


def write_wav(path, samples, rate):
    """float waveform in [-1, 1] -> 16-bit PCM mono (as `soundfile.write(..., "PCM_16")`: scaled by 0x7FFF, rounded to nearest; clipped here)."""
    pcm = np.clip(np.rint(np.asarray(samples, dtype=np.float64) * 32767.0), -32768, 32767).astype("<i2")
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(pcm.tobytes())


def decode(gen, feats, outdir, rate, batch_frames=51200, seed=0, depth=2):
    """feats: list of (utt_id, [T', aux] float32 array).  Writes <outdir>/<utt_id>_gen.wav; returns (samples, seconds)."""
    os.makedirs(outdir, exist_ok=True)
    dev = gen.plan.device
    samples_of = gen.samples_of  # per-utterance sample counts are the generator's (frames x hop; hop x (frames - 1) for Griffin-Lim)
    batches = make_batches([m.shape[0] for _, m in feats], batch_frames)

    def write(items):
        for uid, wav in items:
            write_wav(os.path.join(outdir, uid + "_gen.wav"), wav, rate)

    wr = Writer(write, depth + 1)
    with torch.cuda.device(dev):  # the copies' queue on a compute pipe apart from the generator's stream (ops.stream_apart: fcl_hip.h "Compute pipes")
        copy_stream = ops.stream_apart([torch.cuda.current_stream(dev)], device=dev) if os.environ.get("FCL_PLACE_STREAMS", "1") != "0" else torch.cuda.Stream(device=dev)
    slots = [None] * (depth + 1)  # pinned staging, one per batch in flight
    pending, total = [], 0
    t0 = time.perf_counter()

    def harvest(p):
        ids, lens, host, ev = p
        ev.synchronize()
        arr = host.numpy()
        items, s = [], 0
        for uid, n in zip(ids, lens):
            items.append((uid, arr[s : s + samples_of(n)].copy()))
            s += samples_of(n)
        wr.put(items)
        return s

    try:
        with torch.cuda.device(dev):
            for bi, idx in enumerate(batches):
                mels = [feats[i][1] for i in idx]
                lens = [int(m.shape[0]) for m in mels]
                packed = torch.from_numpy(np.ascontiguousarray(np.concatenate(mels), dtype=np.float32)).to(dev, non_blocking=True)
                _, flat = gen.synthesize_packed(packed, lens, seed=seed + bi, return_flat=True)  # the batch's waveforms are views into this one buffer
                n = sum(samples_of(m) for m in lens)
                j = bi % (depth + 1)
                if slots[j] is None or slots[j].numel() < n:
                    slots[j] = torch.empty(max(n, 1 << 20), dtype=torch.float32, pin_memory=True)
                done = torch.cuda.Event()
                done.record()
                with torch.cuda.stream(copy_stream):
                    copy_stream.wait_event(done)
                    host = slots[j][:n]
                    host.copy_(flat[:n], non_blocking=True)
                    flat.record_stream(copy_stream)
                    ev = torch.cuda.Event()
                    ev.record()
                pending.append(([feats[i][0] for i in idx], lens, host, ev))
                while len(pending) > depth:
                    total += harvest(pending.pop(0))
            while pending:
                total += harvest(pending.pop(0))
    finally:  # the thread is joined also when synthesis fails
        wr.join()
    torch.cuda.synchronize()
    wr.close()  # the writer's first error, if it had one
    return total, time.perf_counter() - t0


def build_parser():
    from . import griffinlim

    ap = argparse.ArgumentParser(prog="fcl_taco2_amd.vocoder_decode",
                                 description="Parallel WaveGAN / HiFi-GAN / Griffin-Lim decoding on MI355X (drop-in for `parallel-wavegan-decode`)")
    ap.add_argument("--checkpoint", default=None, help="generator checkpoint ({'model': {'generator': state_dict}} or a bare state_dict); this or --griffin-lim")
    ap.add_argument("--griffin-lim", action="store_true", help="no checkpoint: pseudo-inverse mel filterbank + Griffin-Lim (exclusive with --checkpoint)")
    ap.add_argument("--feats-scp", "--scp", dest="feats_scp", required=True, help="Kaldi scp of [T', aux] float matrices (decode.py's <out>.scp)")
    ap.add_argument("--outdir", required=True)
    ap.add_argument("--config", default=None, help="parallel_wavegan config.yml (default: next to the checkpoint; v1 geometry without one)")
    ap.add_argument("--batch-frames", type=int, default=51200, help="mel frames per GPU batch")
    ap.add_argument("--nj", type=int, default=1, help="number of utterance shards (one process per GPU)")
    ap.add_argument("--job", type=int, default=0, help="this process's shard (0-based)")
    ap.add_argument("--seed", type=int, default=0, help="seed of the device noise (Griffin-Lim: of the initial phase)")
    ap.add_argument("--verbose", type=int, default=1)
    ap.add_argument("--unsafe-pickle", action="store_true", help="allow the full unpickler for checkpoints that weights_only=True rejects (runs code "
                    "embedded in the file: trusted checkpoints only)")
    griffinlim.add_arguments(ap)
    return ap


def parse_args(argv=None):
    """Parses and checks what can be checked before the first device call; flag errors end in ap.error (SystemExit 2)."""
    from . import griffinlim

    ap = build_parser()
    args = ap.parse_args(argv)
    griffinlim.check_arguments(ap, args, args.checkpoint)
    return args


def main(argv=None):
    args = parse_args(argv)
    torch.set_num_threads(4)
    logging.basicConfig(level=logging.INFO if args.verbose else logging.WARN, format="%(asctime)s %(levelname)s: %(message)s")
    dev = "cuda:%d" % (args.job % max(torch.cuda.device_count(), 1))
    feats = sorted(kaldi_io.read_scp(args.feats_scp).items())
    if args.griffin_lim:
        from . import griffinlim

        # (utterances too short for the reflection are refused by id before the first device call)
        griffinlim.check_lens([m.shape[0] for _, m in feats], args.n_fft, args.hop, [uid for uid, _ in feats])
        gen, rate = griffinlim.from_args(args, dev, n_mels=int(feats[0][1].shape[1]) if feats and feats[0][1].ndim == 2 and args.mel_basis is None else 80)
    else:
        gen, rate = build_generator(args.checkpoint, dev, args.config, args.unsafe_pickle)
    aux = gen.plan.A
    for uid, m in feats:
        if m.ndim != 2 or m.shape[1] != aux or m.shape[0] < 1:
            raise ValueError("%s: expected a [T', %d] feature matrix, got %r" % (uid, aux, m.shape))
    mine = shard_utterances([m.shape[0] for _, m in feats], args.nj)[args.job]
    samples, secs = decode(gen, [feats[i] for i in mine], args.outdir, rate, args.batch_frames, args.seed)
    audio = samples / float(rate)
    logging.info("generated %d utterances, %.1f s of audio in %.2f s (RTF = %.5f)", len(mine), audio, secs, secs / max(audio, 1e-9))
    return samples, secs


if __name__ == "__main__":
    main()
