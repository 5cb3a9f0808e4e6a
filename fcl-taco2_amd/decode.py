"""Decode driver on the HIP path — the role of the reference's `tts_decode.py` + `tts.decode` /
`tts_distill.decode` (tts.py:605-686, tts_distill.py:626-718) with the same inputs and outputs:

  * `--model-conf model.json`  = `[idim, odim, vars(train_args)]` as written by the reference (tts.py:341-348);
    `model_module` values of the reference (`nets....:Tacotron2_sa`) are mapped onto this package's classes;
  * `--model` = `snapshot.ep.N` / `model.loss.best` (ESPnet snapshot: dict with a "model" entry, or a bare state_dict)
    or `amp_checkpoint_*.pt` (`{"model", "optimizer", "amp"}`, tts.py:193-198);
  * `--json` = the data manifest (`{"utts": {id: {"output": [{"tokenid": "1 2 3"}, ...]}}}`, preprocess.py make_json);
  * `--out PREFIX` -> PREFIX.ark / PREFIX.scp (Kaldi float matrices, one mel per utterance) and the mean
    frames / second (stream-synchronised, unlike the reference's unsynchronised clock, tts.py:665-667).
Differences: utterances are synthesised `--batch-size` at a time (sorted by length), and `--nj/--job` shard the manifest
by utterance (what `splitjson.py` + one process per split did), one process per GPU, no collective.
decode() keeps the submit loop (`depth` BatchRunners per length bucket on the shared pass streams); the bucket policy, the capacity sizing and the
writer thread it shares with tts.py are batching.py's (BucketStore, _grown_caps / _ScaledMaps / widened_caps, Writer).
"""
import argparse
import collections
import importlib
import json
import logging
import os
import sys
import threading
import time

import numpy as np
import torch

from .batching import BucketStore, NullArk, Writer, _grown_caps, _ScaledMaps, chunk_selectors, take, widened_caps  # noqa: F401 (sizing: re-exported)
from .kaldi_io import ArkScpWriter
from .prosody import FIELDS as PROSODY_FIELDS, ProsodyControl
from .sharding import shard_utterances

MODULE_MAP = {
    "nets.teacher_training.e2e_tts_tacotron2_sa": "fcl_taco2_amd.nets.teacher_training.e2e_tts_tacotron2_sa",
    "nets.knowledge_distillation.e2e_tts_tacotron2_sa_kd_student": "fcl_taco2_amd.nets.knowledge_distillation.e2e_tts_tacotron2_sa_kd_student",
    "nets.knowledge_distillation.e2e_tts_tacotron2_sa_kd_teacher": "fcl_taco2_amd.nets.knowledge_distillation.e2e_tts_tacotron2_sa_kd_teacher",
}


def get_model_conf(conf_path):
    """model.json -> (idim, odim, Namespace)   (espnet.asr.asr_utils.get_model_conf)."""
    with open(conf_path, "rb") as f:
        idim, odim, args = json.load(f)
    return idim, odim, argparse.Namespace(**args)


def dynamic_import(path):
    mod, cls = path.split(":")
    return getattr(importlib.import_module(MODULE_MAP.get(mod, mod)), cls)


def load_state_dict(path):
    obj = torch.load(path, map_location="cpu", weights_only=False)
    if isinstance(obj, dict) and "model" in obj and isinstance(obj["model"], dict):
        obj = obj["model"]  # ESPnet snapshot or apex-AMP checkpoint
    return {k[len("module."):] if k.startswith("module.") else k: v for k, v in obj.items()}


def build_model(model_path, conf_path, teacher_conf=None, device="cuda:0", share_proj=None):
    idim, odim, train_args = get_model_conf(conf_path)
    cls = dynamic_import(train_args.model_module)
    com = argparse.Namespace(use_fe_condition=True, append_position=True, distill_output_knowledge=True, distill_encoder_knowledge=True,
                             distill_decoder_knowledge=True, distill_prosody_knowledge=True, is_train=True,
                             share_proj=bool(getattr(train_args, "share_proj", False)) if share_proj is None else share_proj)
    train_args.encoder_resume = None
    if cls.role == "student":
        targs = get_model_conf(teacher_conf)[2] if teacher_conf else argparse.Namespace(use_residual=False)
        model = cls(idim, odim, train_args, com, targs)
    else:
        model = cls(idim, odim, train_args, com)
    model.load_state_dict(load_state_dict(model_path))
    return model.eval().to(device)


def read_manifest(json_path):
    with open(json_path, "rb") as f:
        js = json.load(f)["utts"]
    utts = []
    for k, v in js.items():
        ids = np.array(list(map(int, v["output"][0]["tokenid"].split())), dtype=np.int64)
        # speaker embedding: `--use-speaker-embedding` data (tts.py:327-332, 285-287).  A preprocessing manifest's input[1] is the durations file
        # (filetype "npy", manifest.py): no embedding
        if len(v.get("input", [])) > 1 and "feat" in v["input"][1] and v["input"][1].get("filetype") != "npy":
            from .kaldi_io import read_vec

            path, off = v["input"][1]["feat"].rsplit(":", 1)
            utts.append((k, ids, read_vec(path, int(off))))
        else:
            utts.append((k, ids))
    return utts


class _Slot(object):
    """One pinned landing area of a runner's outputs (mel buffer, frame starts, status word); `free` is set by the writer thread once the ark
    holds its utterances, and waited on before the next device-to-host copy may overwrite it."""

    def __init__(self, frames_cap, odim, batch, slab=None):
        """slab: a pinned float32 tensor of at least words(frames_cap, odim, batch) elements to carve the three buffers from (round 6: one pinned allocation
        per bucket instead of three per slot -- 96 hipHostMalloc calls of a first decode() call -> 4)."""
        if slab is None:
            slab = torch.empty(self.words(frames_cap, odim, batch), dtype=torch.float32, pin_memory=True)
        self.whole = slab[: self.words(frames_cap, odim, batch)]  # the layout of BatchRunner.out: one device-to-host copy fills all three
        n = frames_cap * odim
        self.mel = slab[:n].view(frames_cap, odim)
        self.f0 = slab[n : n + batch + 1].view(torch.int32)
        self.st = slab[n + batch + 1 : n + batch + 2].view(torch.int32)
        self.free = threading.Event()
        self.free.set()

    @staticmethod
    def words(frames_cap, odim, batch):
        from .engine import packed_words

        return packed_words(frames_cap, odim, batch)


class _Pool(object):
    """The capacity graphs of one phoneme-length bucket: BatchRunners (predicted durations, created on first use) sharing the bucket's
    capacities; kept on the plan, so later decode() calls on the same model replay the graphs captured by earlier ones."""

    def __init__(self, plan, batch, t_cap, caps, streams, seed, controls=False):
        self.plan, self.batch, self.caps, self.t_cap, self.streams, self.seed = plan, batch, caps, t_cap, streams, seed
        self.controls = controls  # the runners take prosody controls (BatchRunner(controls=True))
        self.runners, self.slots, self.next, self.grow = [None] * len(streams), [None] * len(streams), 0, None
        self._slab = None

    def runner(self, j):
        from . import engine

        if self.runners[j] is None:
            pools_ = self.plan.__dict__.setdefault("_decode_cache", {}).setdefault("graph_mempools", {})
            mp = pools_.setdefault(self.streams[j].cuda_stream, torch.cuda.graph_pool_handle()) if SHARE_GRAPH_POOLS else None  # one per pass stream (stream-ordered graphs)
            r = self.runners[j] = engine.BatchRunner(self.plan, self.batch, self.t_cap, self.caps, forced=False, stream=self.streams[j], seed=self.seed + 7919 * j,
                                                     pack_outputs=True, mempool=mp, controls=self.controls)
            odim = int(r.mel.shape[1])
            w = _Slot.words(self.caps.frames, odim, self.batch)
            if self._slab is None:  # the landing areas of every runner of the bucket: one pinned allocation
                self._slab = torch.empty(2 * len(self.streams) * w, dtype=torch.float32, pin_memory=True)
            self.slots[j] = [_Slot(self.caps.frames, odim, self.batch, self._slab[(2 * j + q) * w : (2 * j + q + 1) * w]) for q in range(2)]
        return self.runners[j]

    def retire(self):
        """Before the bucket is dropped: later captures on its pass streams open a fresh shared memory pool.  (A pool whose last graph is destroyed stays
        in the allocator at use count 0 until its blocks are freed, and a capture into that handle fails the allocator's `use_count > 0` assertion.)"""
        shared = self.plan.__dict__.get("_decode_cache", {}).get("graph_mempools", {})
        for j, r in enumerate(self.runners):
            if r is not None:
                shared.pop(self.streams[j].cuda_stream, None)


grown_caps, ScaledMaps = _grown_caps, _ScaledMaps  # (the names bench.py and earlier callers know; the sizing itself lives in batching.py)


SHARE_GRAPH_POOLS = os.environ.get("FCL_DECODE_SHARE_POOLS", "1") not in ("", "0")  # the graphs of one pass stream share a memory pool (first call: fewer allocations)
ESTIMATE_CAPS = os.environ.get("FCL_DECODE_ESTIMATE_CAPS", "1") not in ("", "0")  # capacities of later buckets from phoneme counts (0: one eager batch per bucket)
MAX_BUCKETS = 8  # captured-graph pools kept per (batch size, depth): least recently used buckets are released beyond this


def release_graphs(model_or_plan):
    """Drop every captured decode graph (and its pinned landing buffers) kept on the model's plan by earlier decode() calls."""
    plan = model_or_plan.plan() if hasattr(model_or_plan, "plan") and callable(model_or_plan.plan) else model_or_plan
    plan.__dict__.pop("_decode_cache", None)


@torch.no_grad()
def decode(model, utts, out_prefix, batch_size=32, seed=137, depth=4, stats=None, keep_graphs=True, max_buckets=None, prosody=None):
    """utts: [(utt_id, ids)] or, for a model with spk_embed_dim, [(utt_id, ids, spemb)].  Writes PREFIX.ark/.scp (out_prefix None: nothing is written); returns (frames, seconds).
    Every batch runs as ONE captured graph with predicted durations (engine.BatchRunner): the host packs the phoneme ids, enqueues one
    graph launch (its first node pulls the packed block into HBM) and one D2H copy of the mel buffer + the per-utterance frame starts, and only synchronises on a batch when it
    harvests it `depth` batches later -- no read-back of the predicted durations in the middle of a pass (rounds 1-2 did one per batch).  The
    mels go from the pinned landing buffer straight into the ark on a writer thread (no intermediate copy on the submitting thread).
    Utterances are sorted by length and bucketed by padded phoneme count (multiples of 16); the first batch of a bucket runs eagerly with the
    host round trip, which both produces its mels and calibrates the bucket's capacities (decoder steps, frames, live rows per step, with
    slack); a later batch that exceeds them is reported by the device (FCL_STATUS_*), re-run eagerly, and the bucket's capacities grow.  The
    captured graphs stay with the model's plan: a second decode() on the same model replays them -- at most `max_buckets` (MAX_BUCKETS) length
    buckets per (batch size, depth), least recently used first out (each holds up to `depth` graphs with private memory pools and two pinned
    landing buffers per graph); keep_graphs=False releases all of them when the call returns (release_graphs() does it later).
    An error inside the loop (a zero-duration phoneme raising like the reference, a failing writer) still drains the device, stops the writer
    thread and closes the ark before it propagates.
    stats (dict, optional): receives `device_seconds` — first submit -> last batch complete on the GPU, excluding the ark writing.
    prosody: None, one prosody.ProsodyControl for every utterance, or a dict {utt_id: ProsodyControl or {field: value}} (utterances not named:
    identity).  Controlled runs keep their graphs (BatchRunner(controls=True)) and calibration under keys of their own; the eager
    calibration batch of a bucket runs with its controls, so the capacities follow the duration scale."""
    from . import engine, ops

    torch.manual_seed(seed)
    order = sorted(range(len(utts)), key=lambda i: -len(utts[i][1]))
    dev = next(model.parameters()).device
    plan = model.plan(dev)
    spk_of, ctl_of, controlled = chunk_selectors(plan, utts, prosody)
    ckey = ("ctl",) if controlled else ()  # controlled graphs and calibrations never replace the uncontrolled ones
    frames = 0
    depth = max(1, int(depth))
    cache = plan.__dict__.setdefault("_decode_cache", {})
    streams = engine.shared_streams(dev, depth)  # the process's pass streams (one pool per device: see engine.shared_streams)
    pending = []
    n_eager = n_graph = n_redo = 0
    # dlayers / prenet_layers / elayers other than 2 / 2 / 1 run on the fp32-operand loop with host row counts (fcl_decoder_weights_t.dlayers ...)
    eager_only = bool(getattr(plan, "generic_decoder", False)) or plan.hp.elayers != 1

    def eager(chunk):
        """Host-round-trip pass (calibration / fallback): exact maps of THIS batch."""
        prep = engine.prepare(plan, [u[1] for u in chunk], spembs=spk_of(chunk), prosody=ctl_of(chunk))
        mel, utt_frames, inter = engine.run(plan, prep, ops.DROP_RNG, seed=int(torch.randint(0, 2 ** 31 - 1, (1,)).item()), return_intermediates=True)
        arr = mel.cpu().numpy()
        wr.put((chunk, arr, list(utt_frames)))
        return int(arr.shape[0]), inter["maps"]

    def harvest(item):
        nonlocal n_redo
        pool, j, chunk, slot, ev = item
        ev.synchronize()
        if int(slot.st[0]) != 0:  # a capacity of the bucket did not hold for this batch (or a phoneme got duration 0: eager() then raises like the reference)
            pool.runners[j].status.zero_()
            slot.free.set()
            n_redo += 1
            got, pool.grow = eager(chunk)
            return got
        f0 = slot.f0.numpy()
        total = int(f0[len(chunk)])
        wr.put((chunk, slot.mel.numpy()[:total], [int(v) for v in np.diff(f0[: len(chunk) + 1])]), slot.free)
        return total

    def drain(pool):
        """The store is about to drop the bucket: its batches in flight are harvested, the writer thread is done with its pinned landing buffers."""
        nonlocal frames
        for it in take(pending, lambda p: p[0] is pool):
            frames += harvest(it)
        for sl in [x for pair in pool.slots if pair for x in pair]:
            sl.free.wait()
        pool.retire()

    # the pools and the calibration -- [(exact maps, phoneme count)] of the first eagerly calibrated batch of this model -- stay with the plan; `bi` in
    # make is the batch the loop below is at when the policy asks for a bucket
    store = BucketStore(engine, batch_size, lambda t_cap, caps: _Pool(plan, batch_size, t_cap, caps, streams, seed + 31 * bi, controlled), drain,
                        MAX_BUCKETS if max_buckets is None else max_buckets, ESTIMATE_CAPS,
                        cache.setdefault(("pools", batch_size, depth) + ckey, collections.OrderedDict()), cache.setdefault(("calibration", batch_size) + ckey, []),
                        sizing=sys.modules[__name__])
    # the ark / scp file is written by a worker thread: out_prefix None = synthesis + device-to-host hand-over only (benchmarks)
    with (ArkScpWriter(out_prefix) if out_prefix is not None else NullArk()) as w, torch.cuda.device(dev):
        wr = Writer(lambda it: w.write_batch([u[0] for u in it[0]], it[1][: int(sum(it[2]))], it[2]), 4 * (depth + 1))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        try:
            for bi, s in enumerate(range(0, len(order), batch_size)):
                chunk = [utts[i] for i in order[s : s + batch_size]]
                if eager_only:  # structure options beyond the shipped recipes: the launch-by-launch pass (no capacity graphs for them)
                    got, _ = eager(chunk)
                    frames += got
                    n_eager += 1
                    continue
                t_cap = (max(len(u[1]) for u in chunk) + 15) // 16 * 16
                n_ph = sum(len(u[1]) for u in chunk)
                pool = store.get(t_cap, n_ph)
                if pool is None:  # first batch of the bucket: eager pass = its result + the bucket's calibration
                    got, maps = eager(chunk)
                    frames += got
                    n_eager += 1
                    store.calibrated(t_cap, maps, n_ph)
                    continue
                j = pool.next % len(streams)
                pool.next += 1
                for it in take(pending, lambda p: p[1] == j):  # stream j's previous batch (of any bucket) must have left the runner's static buffers
                    frames += harvest(it)
                r = pool.runner(j)
                if r.R is not None and n_ph > r.R:  # more phonemes than the bucket's compact rows hold: handled like a capacity the device reports
                    n_redo += 1
                    got, pool.grow = eager(chunk)
                    frames += got
                    continue
                slot = pool.slots[j][(pool.next // len(streams)) % 2]
                slot.free.wait()  # the writer thread is done with what this landing buffer held
                slot.free.clear()
                try:
                    r.load([u[1] for u in chunk], spembs=spk_of(chunk), prosody=ctl_of(chunk))
                except Exception:
                    slot.free.set()
                    raise
                r.replay()
                with torch.cuda.stream(r.stream):
                    if r.out is not None and r.out.numel() == slot.whole.numel():
                        slot.whole.copy_(r.out, non_blocking=True)  # mel | frame starts | status in one call (round 6)
                    else:
                        slot.mel.copy_(r.mel, non_blocking=True)
                        slot.f0.copy_(r._frames.utt_frame0, non_blocking=True)
                        slot.st.copy_(r.status, non_blocking=True)
                    ev = torch.cuda.Event()
                    ev.record(r.stream)
                pending.append((pool, j, chunk, slot, ev))
                n_graph += 1
            while pending:
                frames += harvest(pending.pop(0))
            torch.cuda.synchronize()
            dev_secs = time.perf_counter() - t0
        except BaseException:
            # graphs already launched keep copying into the pinned landing buffers: wait for the device, hand the slots back, and let the
            # writer finish what it was given -- then the ark is closed by the `with` and the error propagates
            torch.cuda.synchronize()
            for it in take(pending):
                it[0].runners[it[1]].status.zero_()
                it[3].free.set()
            raise
        finally:
            wr.join()
            if not keep_graphs:
                release_graphs(plan)
        secs = time.perf_counter() - t0
        wr.close()  # the writer's first error, if it had one
    if stats is not None:
        stats.update(device_seconds=dev_secs, eager_batches=n_eager, graph_batches=n_graph, redone_batches=n_redo, buckets=len(store.buckets),
                     evicted_buckets=store.evicted, estimated_buckets=store.estimated)
    return frames, secs


def add_prosody_arguments(ap):
    g = ap.add_argument_group("prosody control (edits the predicted durations / pitch / energy; INTEGRATION.md)")
    g.add_argument("--duration-scale", type=float, default=None, help="speaking-rate factor on the predicted durations, in (0, 8] (2: twice as long)")
    g.add_argument("--pitch-scale", type=float, default=None, help="scale of the normalised pitch")
    g.add_argument("--pitch-shift", type=float, default=None, help="shift of the normalised pitch")
    g.add_argument("--energy-scale", type=float, default=None, help="scale of the normalised energy")
    g.add_argument("--energy-shift", type=float, default=None, help="shift of the normalised energy")
    g.add_argument("--semitones", type=float, default=None, help="pitch shift in semitones (needs --f0-en-stats)")
    g.add_argument("--pitch-range", type=float, default=None, help="pitch-range factor (same as --pitch-scale)")
    g.add_argument("--energy-gain", type=float, default=None, help="energy gain on the linear energy (needs --f0-en-stats)")
    g.add_argument("--f0-en-stats", default=None, help="f0_en_stats.npy of preprocessing: [f0_mean, f0_std, en_mean, en_std]")
    g.add_argument("--prosody-json", default=None, help="per-utterance controls {utt_id: {field: value}} on top of the global ones")


def prosody_from_args(args, utt_ids=None):
    """The decode flags -> None (no control), one ProsodyControl, or {utt_id: ProsodyControl}.  Raises ValueError on inconsistent flags."""
    raw = {f: getattr(args, f) for f in PROSODY_FIELDS if getattr(args, f) is not None}
    units = {k: getattr(args, k) for k in ("semitones", "pitch_range", "energy_gain") if getattr(args, k) is not None}
    if ("semitones" in units or "pitch_range" in units) and ("pitch_scale" in raw or "pitch_shift" in raw):
        raise ValueError("--semitones / --pitch-range and --pitch-scale / --pitch-shift both set the pitch control: give one of them")
    if "energy_gain" in units and ("energy_scale" in raw or "energy_shift" in raw):
        raise ValueError("--energy-gain and --energy-scale / --energy-shift both set the energy control: give one of them")
    if ("semitones" in units or "energy_gain" in units) and args.f0_en_stats is None:
        raise ValueError("--semitones / --energy-gain need --f0-en-stats (the pitch / energy statistics of preprocessing)")
    base = dict(raw)
    if units:
        u = ProsodyControl.from_units(stats=args.f0_en_stats, semitones=units.get("semitones", 0.0), pitch_range=units.get("pitch_range", 1.0),
                                      energy_gain=units.get("energy_gain", 1.0))
        if "semitones" in units or "pitch_range" in units:
            base.update(pitch_scale=u.pitch_scale, pitch_shift=u.pitch_shift)
        if "energy_gain" in units:
            base.update(energy_scale=u.energy_scale, energy_shift=u.energy_shift)
    glob = ProsodyControl(**base)  # validates
    if args.prosody_json is None:
        return glob if base else None
    with open(args.prosody_json) as f:
        per = json.load(f)
    if not isinstance(per, dict) or not all(isinstance(v, dict) for v in per.values()):
        raise ValueError("--prosody-json: expected {utt_id: {field: value}}")
    out = {k: ProsodyControl.coerce(dict(base, **v)) for k, v in per.items()}
    for k in (utt_ids or ()):
        out.setdefault(k, glob)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description="FCL-taco2 mel synthesis on MI355X (reference-compatible decode driver)")
    ap.add_argument("--model", required=True)
    ap.add_argument("--model-conf", required=True)
    ap.add_argument("--teacher-config", default=None, help="model.json of the teacher (student checkpoints trained with KD projections)")
    ap.add_argument("--json", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--nj", type=int, default=1, help="number of utterance shards (one process per GPU)")
    ap.add_argument("--job", type=int, default=0, help="this process's shard (0-based)")
    ap.add_argument("--seed", type=int, default=137)
    ap.add_argument("--verbose", type=int, default=1)
    add_prosody_arguments(ap)
    args = ap.parse_args(argv)
    try:
        prosody_from_args(args)  # flag errors before anything is loaded
    except ValueError as e:
        ap.error(str(e))
    torch.set_num_threads(4)  # kernels are launched from this thread; a one-thread-per-core intra-op pool spinning beside it slows them
    logging.basicConfig(level=logging.INFO if args.verbose else logging.WARN, format="%(asctime)s %(levelname)s: %(message)s")
    dev = "cuda:%d" % (args.job % max(torch.cuda.device_count(), 1))
    model = build_model(args.model, args.model_conf, args.teacher_config, dev)
    utts = read_manifest(args.json)
    mine = shard_utterances([len(u[1]) for u in utts], args.nj)[args.job]
    out = args.out if args.nj == 1 else "%s.%d" % (args.out, args.job + 1)
    prosody = prosody_from_args(args, [utts[i][0] for i in mine])
    frames, secs = decode(model, [utts[i] for i in mine], out, args.batch_size, args.seed, prosody=prosody)
    logging.info("average inference speed = %.1f frames / sec. (%d utterances, %d frames)", frames / max(secs, 1e-9), len(mine), frames)
    return frames, secs


if __name__ == "__main__":
    main()
