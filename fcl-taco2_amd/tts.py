"""Text -> waveform in one process on MI355X: the reference's two-step recipe (inference_student.sh: `tts_decode.py` writes mels as ark/scp,
`parallel-wavegan-decode` reads them back in a second process) as ONE driver, one captured graph per batch.

    python -m fcl_taco2_amd.tts --model exp/student/results/model.last1.avg.best --model-conf exp/student/results/model.json \\
        --json dump/test/data.json --vocoder-checkpoint vocoder/PWG/PWG.pkl --outdir exp/student/test/wav

Writes `<outdir>/<utt_id>_gen.wav` (16-bit PCM mono at the vocoder config's sampling rate), what the two-step recipe writes.  Utterances are
sorted by length and bucketed by padded phoneme count like decode.py; every bucket keeps one engine.SpeechRunner (synthesis with predicted
durations -> capacity vocoder -> int16 PCM in a single hipGraph; the durations never reach the host).  Capacities follow the bucket policy
decode.py follows too (batching.BucketStore): the first batch runs through the two-step route (synthesis, frame counts on the host, exact-size vocoder), which both produces its
audio and calibrates; later buckets are estimated from their phoneme counts; a batch that overflows a capacity is reported by the device, redone
through the two-step route, and its bucket grows.  The int16 PCM travels through pinned staging on a placed copy stream while the next batch
runs; a writer thread (batching.Writer) encodes the wav files.  `--feats-out PREFIX` also writes the mels the waveforms were made from as PREFIX.ark/.scp, so a
run can be audited against `decode.py` + `vocoder_decode.py`.

One SpeechRunner holds 1082 bytes per capacity sample (vocoder.CapacitySynth), 10.4 GB at the measured BASELINE configs[4] capacity (64
utterances of 60 - 100 phonemes, 37 632 frames: DESIGN.md 6b), so few are kept: `--max-buckets` (default 2), least recently used first out.
A HiFi-GAN generator takes the two-step route for every batch by default; `--vocoder-graph` puts it on the same one-graph route through its
capacity form (hifigan.CapacitySynth, ~0.94 KB per capacity sample for v1: DESIGN.md 6c).  `--griffin-lim` instead of `--vocoder-checkpoint` needs no
trained generator (griffinlim.py); it has no capacity form, every batch takes the two-step route, and an utterance of T' frames gives
hop * (T' - 1) samples."""
import argparse
import logging
import os
import threading
import time
import wave

import numpy as np
import torch

from .batching import BucketStore, NullArk, Writer, chunk_selectors, take
from .decode import add_prosody_arguments, build_model, prosody_from_args, read_manifest
from .kaldi_io import ArkScpWriter
from .sharding import shard_utterances

MAX_BUCKETS = 2


def bucket_of(n_phonemes):
    """Padded phoneme count of a batch whose longest utterance has n_phonemes: the next multiple of 16 (decode.py's buckets)."""
    return (int(n_phonemes) + 15) // 16 * 16


def plan_batches(lengths, batch_size):
    """Utterance indices sorted by phoneme count (longest first, stable), cut into batches of `batch_size` -> [(t_cap, [indices])]."""
    if batch_size < 1:
        raise ValueError("--batch-size must be at least 1 (got %d)" % batch_size)
    order = sorted(range(len(lengths)), key=lambda i: -int(lengths[i]))
    return [(bucket_of(max(int(lengths[i]) for i in order[s : s + batch_size])), order[s : s + batch_size]) for s in range(0, len(order), batch_size)]


def vocoder_frames_cap(caps_frames, hop):
    """The vocoder's frame capacity behind a synthesis pass of `caps_frames` frames: the same count, refused when its samples leave int32."""
    if int(caps_frames) * int(hop) >= 2 ** 31 - 1:
        raise ValueError("fcl-taco2_amd: a batch capacity of %d frames x hop %d exceeds 2^31 samples: use a smaller --batch-size" % (caps_frames, hop))
    return int(caps_frames)


def write_pcm_wav(path, pcm, rate):
    """int16 samples -> 16-bit PCM mono wav (the bytes vocoder_decode.write_wav writes for the float waveform they were rounded from)."""
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(int(rate))
        w.writeframes(np.ascontiguousarray(pcm, dtype="<i2").tobytes())


class _Bucket(object):
    """One phoneme-length bucket: its capacities, its SpeechRunner (created on first use) and two pinned landing areas."""

    def __init__(self, t_cap, caps):
        self.t_cap, self.caps, self.runner, self.slots, self.next, self.grow, self.copied, self.replays = t_cap, caps, None, None, 0, None, None, 0


@torch.no_grad()
def synthesize(model, gen, utts, outdir, rate, batch_size=32, seed=137, prosody=None, feats_out=None, max_buckets=None, vocoder_graph=False):
    """utts: [(utt_id, ids)] or [(utt_id, ids, spemb)].  Writes <outdir>/<utt_id>_gen.wav; returns a dict: samples, seconds, rtf, utterances and
    how many batches took each route (graph_batches, eager_batches, redone_batches; their sum is the number of batches), and `batches`: per batch
    (route, utterance ids in batch order, vocoder noise seed).  vocoder_graph: a generator whose default route is the two-step one but which has a
    capacity form (HiFi-GAN: gen.capacity_synth) takes the bucketed one-graph route too; nothing changes for Parallel WaveGAN."""
    from . import engine, ops, vocoder

    os.makedirs(outdir, exist_ok=True)
    torch.manual_seed(seed)
    dev = next(model.parameters()).device
    plan = model.plan(dev)
    hop, odim = gen.plan.hop, int(plan.hp.odim)
    if odim != gen.plan.A:
        raise ValueError("fcl-taco2_amd: the model writes %d mel channels, the vocoder takes %d" % (odim, gen.plan.A))
    spk_of, ctl_of, controlled = chunk_selectors(plan, utts, prosody)
    # (a generator whose default route is the two-step one -- HiFi-GAN -- keeps every batch on it, like a model the capacity graph does not cover,
    # unless the caller asks for the graph route and the generator has a capacity form)
    gen_eager = bool(getattr(gen.plan, "eager_only", False)) and not (vocoder_graph and hasattr(gen, "capacity_synth"))
    eager_only = bool(getattr(plan, "generic_decoder", False)) or plan.hp.elayers != 1 or gen_eager
    counts = dict(graph_batches=0, eager_batches=0, redone_batches=0)
    routes = {}  # batch number -> (route, utterance ids, vocoder noise seed): what an audit needs to redo a batch from its mels

    def write(item):
        chunk, pcm, offs, mel, frames = item
        for i, u in enumerate(chunk):
            write_pcm_wav(os.path.join(outdir, u[0] + "_gen.wav"), pcm[offs[i] : offs[i + 1]], rate)
        if mel is not None:
            ark.write_batch([u[0] for u in chunk], mel[: int(sum(frames))], frames)

    def two_step(chunk, k):
        """Synthesis with the host round trip, then the exact-size vocoder: calibration of a bucket and the redo route."""
        prep = engine.prepare(plan, [u[1] for u in chunk], spembs=spk_of(chunk), prosody=ctl_of(chunk))
        mel, frames, inter = engine.run(plan, prep, ops.DROP_RNG, seed=int(torch.randint(0, 2 ** 31 - 1, (1,)).item()), return_intermediates=True)
        frames = [int(f) for f in frames]
        nseed = (seed + 104729 * k) & 0xFFFFFFFF
        routes[k] = ("two-step", [u[0] for u in chunk], nseed)
        if hasattr(gen, "check_lens"):  # Griffin-Lim: an utterance too short for its reflection is refused by id
            gen.check_lens(frames, [u[0] for u in chunk])
        _, flat = gen.synthesize_packed(mel, frames, seed=nseed, return_flat=True)
        offs = np.concatenate([[0], np.cumsum([gen.samples_of(f) for f in frames])])  # (frames x hop; hop x (frames - 1) for Griffin-Lim)
        n = int(offs[-1])
        host = vocoder.pcm16(flat)
        wr.put((chunk, host, offs, mel.cpu().numpy() if feats_out else None, frames))
        return n, inter["maps"]

    def harvest(item):
        b, chunk, slot, ev, k = item
        ev.synchronize()
        bits = int(slot["st"][0]) & 0xFFFFFFFF
        if bits:  # a capacity of the bucket did not hold for this batch (a zero duration raises from the two-step route like the reference)
            slot["free"].set()  # (the runner's own word is cleared on ITS stream in front of its next replay, never from here)
            counts["redone_batches"] += 1
            counts["graph_batches"] -= 1
            logging.info("batch %d: %s -- redone through the two-step route", k, ops.status_message(bits))
            got, b.grow = two_step(chunk, k)
            return got
        f0 = slot["f0"].numpy().astype(np.int64)
        frames = [int(v) for v in np.diff(f0[: len(chunk) + 1])]
        wr.put((chunk, slot["pcm"].numpy(), f0 * hop, slot["mel"].numpy() if feats_out else None, frames), slot["free"])
        return int(f0[len(chunk)]) * hop

    def make(t_cap, caps):
        vocoder_frames_cap(caps.frames, hop)
        return _Bucket(t_cap, caps)

    pending, samples = [], 0

    def drain(b):
        nonlocal samples
        for it in take(pending, lambda p: p[0] is b):
            samples += harvest(it)
        for sl in (b.slots or []):
            sl["free"].wait()

    # the buckets and the calibration of the run (the first batch's exact maps) live for this call only
    store = BucketStore(engine, batch_size, make, drain, MAX_BUCKETS if max_buckets is None else max_buckets)
    with (ArkScpWriter(feats_out) if feats_out else NullArk()) as ark, torch.cuda.device(dev):
        main_stream = engine.shared_streams(dev, 1)[0]
        copy_stream = ops.stream_apart([main_stream], device=dev) if os.environ.get("FCL_PLACE_STREAMS", "1") != "0" else torch.cuda.Stream(device=dev)
        wr = Writer(write, 8)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        try:
            for k, (t_cap, idx) in enumerate(plan_batches([len(u[1]) for u in utts], batch_size)):
                chunk = [utts[i] for i in idx]
                if eager_only:
                    samples += two_step(chunk, k)[0]
                    counts["eager_batches"] += 1
                    continue
                n_ph = sum(len(u[1]) for u in chunk)
                b = store.get(t_cap, n_ph)
                if b is None:  # the first batch of the run: the two-step route = its audio + the calibration
                    got, maps = two_step(chunk, k)
                    samples += got
                    counts["eager_batches"] += 1
                    store.calibrated(t_cap, maps, n_ph)
                    continue
                if b.runner is None:
                    b.runner = engine.SpeechRunner(plan, gen, batch_size, t_cap, b.caps, forced=False, stream=main_stream, seed=seed + 31 * k,
                                                   controls=controlled)
                    r = b.runner
                    mk = lambda: dict(pcm=torch.empty(r.synth.M, dtype=torch.int16, pin_memory=True), f0=torch.empty(batch_size + 1, dtype=torch.int32, pin_memory=True),
                                      st=torch.empty(1, dtype=torch.int32, pin_memory=True), free=threading.Event(),
                                      mel=torch.empty(tuple(r.mel.shape), dtype=torch.float32, pin_memory=True) if feats_out else None)
                    b.slots = [mk(), mk()]
                    for sl in b.slots:
                        sl["free"].set()
                r = b.runner
                if r.R is not None and n_ph > r.R:  # more phonemes than the bucket's compact rows hold: handled like a capacity the device reports
                    counts["redone_batches"] += 1
                    logging.info("batch %d: %d phonemes, row capacity %d -- redone through the two-step route", k, n_ph, r.R)
                    got, b.grow = two_step(chunk, k)
                    samples += got
                    continue
                slot = b.slots[b.next % 2]
                b.next += 1
                for it in take(pending, lambda p: p[2] is slot):  # this landing area's previous batch
                    samples += harvest(it)
                slot["free"].wait()
                slot["free"].clear()
                try:
                    r.load([u[1] for u in chunk], spembs=spk_of(chunk), prosody=ctl_of(chunk))
                except Exception:
                    slot["free"].set()
                    raise
                # Two batches of one runner are in flight (one running, one on its way to the host), but its status word and static buffers have ONE
                # owner at a time, in stream order: the previous batch's copies (PCM, frame starts, status, mel) -> this wait -> the word cleared on
                # the runner's stream -> this batch's graph.  Each batch is judged by its own copied word only; nobody clears the word from the host side.
                if b.copied is not None:
                    r.stream.wait_event(b.copied)
                with torch.cuda.stream(r.stream):
                    r.status.zero_()
                r.replay()
                b.replays += 1  # (= the runner's device seed word after this replay)
                routes[k] = ("graph", [u[0] for u in chunk], (r.seed + b.replays) & 0xFFFFFFFF)
                done = torch.cuda.Event()
                done.record(r.stream)
                with torch.cuda.stream(copy_stream):
                    copy_stream.wait_event(done)
                    slot["pcm"].copy_(r.pcm, non_blocking=True)
                    slot["f0"].copy_(r._frames.utt_frame0[: batch_size + 1], non_blocking=True)
                    slot["st"].copy_(r.status, non_blocking=True)
                    if feats_out:
                        slot["mel"].copy_(r.mel, non_blocking=True)
                    ev = torch.cuda.Event()
                    ev.record(copy_stream)
                b.copied = ev
                pending.append((b, chunk, slot, ev, k))
                counts["graph_batches"] += 1
            while pending:
                samples += harvest(pending.pop(0))
            torch.cuda.synchronize()
        except BaseException:
            torch.cuda.synchronize()
            for it in take(pending):
                it[2]["free"].set()
            raise
        finally:
            wr.join()
        secs = time.perf_counter() - t0
        wr.close()  # the writer's first error, if it had one
    audio = samples / float(rate)
    return dict(samples=int(samples), seconds=secs, rtf=secs / max(audio, 1e-9), utterances=len(utts), batches=[routes[k] for k in sorted(routes)], **counts)


def build_parser():
    from . import griffinlim

    ap = argparse.ArgumentParser(prog="fcl_taco2_amd.tts", description="FCL-taco2 text -> waveform on MI355X in one process (synthesis + Parallel WaveGAN)")
    ap.add_argument("--model", required=True)
    ap.add_argument("--model-conf", required=True)
    ap.add_argument("--teacher-config", default=None, help="model.json of the teacher (student checkpoints trained with KD projections)")
    ap.add_argument("--json", required=True, help="data.json manifest (phoneme ids per utterance)")
    ap.add_argument("--vocoder-checkpoint", default=None, help="generator checkpoint ({'model': {'generator': state_dict}} or a bare state_dict); this or "
                    "--griffin-lim")
    ap.add_argument("--griffin-lim", action="store_true", help="no vocoder checkpoint: pseudo-inverse mel filterbank + Griffin-Lim (exclusive with "
                    "--vocoder-checkpoint; every batch takes the two-step route)")
    ap.add_argument("--vocoder-config", default=None, help="parallel_wavegan config.yml (default: next to the checkpoint; v1 geometry without one)")
    ap.add_argument("--outdir", required=True)
    ap.add_argument("--feats-out", default=None, metavar="PREFIX", help="also write the mels as PREFIX.ark / PREFIX.scp")
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--max-buckets", type=int, default=MAX_BUCKETS, help="captured text->waveform graphs kept (each holds ~1.07 KB per capacity sample with "
                    "Parallel WaveGAN, ~0.94 KB with HiFi-GAN v1)")
    ap.add_argument("--vocoder-graph", action="store_true", help="HiFi-GAN: run the generator inside the captured text->waveform graph (its capacity form) "
                    "instead of the two-step route; no effect for Parallel WaveGAN, which always does")
    ap.add_argument("--nj", type=int, default=1, help="number of utterance shards (one process per GPU)")
    ap.add_argument("--job", type=int, default=0, help="this process's shard (0-based)")
    ap.add_argument("--seed", type=int, default=137)
    ap.add_argument("--verbose", type=int, default=1)
    ap.add_argument("--unsafe-pickle", action="store_true", help="allow the full unpickler for vocoder checkpoints that weights_only=True rejects (runs code "
                    "embedded in the file: trusted checkpoints only)")
    add_prosody_arguments(ap)
    griffinlim.add_arguments(ap)
    return ap


def parse_args(argv=None):
    """Parses and checks everything that can be checked before the first device call; flag errors end in ap.error (SystemExit 2)."""
    from . import griffinlim

    ap = build_parser()
    args = ap.parse_args(argv)
    griffinlim.check_arguments(ap, args, args.vocoder_checkpoint)
    if args.batch_size < 1:
        ap.error("--batch-size must be at least 1")
    if args.nj < 1 or not 0 <= args.job < args.nj:
        ap.error("--job must lie in [0, --nj) (got --job %d --nj %d)" % (args.job, args.nj))
    if args.max_buckets < 1:
        ap.error("--max-buckets must be at least 1")
    try:
        prosody_from_args(args)
    except ValueError as e:
        ap.error(str(e))
    return args


def shard_of(utts, nj, job):
    """This job's utterances (balanced by phoneme count, like decode.py)."""
    return [utts[i] for i in shard_utterances([len(u[1]) for u in utts], nj)[job]]


def main(argv=None):
    args = parse_args(argv)
    from .vocoder_decode import build_generator

    torch.set_num_threads(4)
    logging.basicConfig(level=logging.INFO if args.verbose else logging.WARN, format="%(asctime)s %(levelname)s: %(message)s")
    dev = "cuda:%d" % (args.job % max(torch.cuda.device_count(), 1))
    model = build_model(args.model, args.model_conf, args.teacher_config, dev)
    if args.griffin_lim:
        from . import griffinlim

        gen, rate = griffinlim.from_args(args, dev, n_mels=int(model.plan(dev).hp.odim))
    else:
        gen, rate = build_generator(args.vocoder_checkpoint, dev, args.vocoder_config, args.unsafe_pickle)
    mine = shard_of(read_manifest(args.json), args.nj, args.job)
    feats = args.feats_out if args.feats_out is None or args.nj == 1 else "%s.%d" % (args.feats_out, args.job + 1)
    res = synthesize(model, gen, mine, args.outdir, rate, args.batch_size, args.seed, prosody_from_args(args, [u[0] for u in mine]), feats, args.max_buckets,
                     vocoder_graph=args.vocoder_graph)
    logging.info("generated %d utterances, %.1f s of audio in %.2f s (RTF = %.5f); batches: %d graph, %d eager, %d redone", res["utterances"],
                 res["samples"] / float(rate), res["seconds"], res["rtf"], res["graph_batches"], res["eager_batches"], res["redone_batches"])
    return res


if __name__ == "__main__":
    main()
