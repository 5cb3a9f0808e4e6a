"""Host-side batching shared by the pipelined drivers (decode.py, tts.py, vocoder_decode.py): the capacity sizing of a length bucket, the bucket
policy (BucketStore: calibrate once, estimate later buckets, widen after an overflow, keep the least recently used ones), the writer thread, and the
per-chunk selection helpers, and the frame-count packing of the drivers that take whole utterances (make_batches: vocoder_decode.py,
extract_features.py).  No device call and no torch in here: the drivers keep their submit loops and hand in what differs (how a bucket is
made, how its batches in flight are harvested), so the policy runs on the CPU with fakes (tests/test_batching.py)."""
import collections
import queue
import sys
import threading

import numpy as np

from .prosody import ProsodyControl


def _grown_caps(engine, maps, n_rows, scale=1.3):
    """Capacities for the batches that follow the one whose exact maps are `maps` (they are no longer than it): some slack on every count."""
    lmax = max(16, int(maps.lmax * 1.5) + 4)
    bounds = np.full(lmax, 1, dtype=np.int32)
    live = np.minimum(n_rows, (maps.live_rows.astype(np.float64) * scale).astype(np.int64) + 32)
    bounds[: maps.lmax] = live
    bounds[maps.lmax :] = live[-1]
    bounds = np.maximum.accumulate(bounds[::-1])[::-1].astype(np.int32)  # non-increasing, as the loop requires
    # the steps past this batch's own longest duration (+ 2) are slack: the rows that do reach them continue in one launch of the row-tile kernel;
    # the phoneme rows (live_rows[0]: every row has a duration above 0) get the live rows' slack and cap: at n_rows the runner keeps the padded layout
    caps = engine.Caps(lmax, (int(maps.n_frames * scale) + 255) // 256 * 256, bounds, tail_from=maps.lmax + 2)
    caps.rows = int(live[0])
    return caps


class _ScaledMaps(object):
    """The exact maps of a calibration batch rescaled to another batch's phoneme count: durations are a per-phoneme quantity, so a later bucket's
    frame total and live-row profile are the calibrated ones x (its phonemes / the calibrated batch's phonemes); _grown_caps adds the slack and a
    batch that still overflows is reported by the device and redone by the host route (bucket.grow)."""

    def __init__(self, maps, n_ph_cal, n_ph):
        ratio = float(n_ph) / float(max(n_ph_cal, 1))
        self.lmax = int(maps.lmax)
        self.live_rows = np.ceil(np.asarray(maps.live_rows, dtype=np.float64) * ratio).astype(np.int64)
        self.n_frames = int(np.ceil(maps.n_frames * ratio))


def widened_caps(engine, maps, old, n_rows):
    """Capacities of a bucket after one of its batches (exact maps `maps`, from its redo) overflowed `old`: more slack on every count, never
    less than before, and every step may keep every row."""
    g = _grown_caps(engine, maps, n_rows, scale=1.6)
    lmax = max(g.lmax, old.lmax)
    return engine.Caps(lmax, max(g.frames, old.frames), np.full(lmax, n_rows, np.int32), tail_from=g.tail_from)


class BucketStore(object):
    """The length buckets of a run, keyed by padded phoneme count, at most `max_buckets` of them, least recently used first out.  A bucket is
    whatever make(t_cap, caps) returns; the store reads its `caps` and its `grow` (None, or the exact maps of a batch that overflowed it).
    drain(bucket) harvests the bucket's batches in flight and waits until the writer has released its landing buffers; it runs before a bucket is
    replaced or dropped.  `buckets` (an OrderedDict) and `calibration` (a list: empty, or [(exact maps, phoneme count)]) may live outside the store,
    so that a later run finds them; `estimated` and `evicted` count this store's own decisions.  The sizing (_grown_caps, _ScaledMaps, widened_caps)
    is looked up at call time on `sizing`: this module, or a module that re-exports the three names (decode.py, where its tests substitute them)."""

    def __init__(self, engine, batch_size, make, drain, max_buckets, estimate=True, buckets=None, calibration=None, sizing=None):
        self.engine, self.batch_size, self.make, self.drain, self.estimate = engine, batch_size, make, drain, estimate
        self.sizing = sys.modules[__name__] if sizing is None else sizing
        self.max_buckets = max(1, int(max_buckets))
        self.buckets = collections.OrderedDict() if buckets is None else buckets
        self.calibration = [] if calibration is None else calibration
        self.estimated = self.evicted = 0

    def get(self, t_cap, n_ph):
        """The bucket for a batch of n_ph phonemes padded to t_cap, or None: run that batch by the host route, then call calibrated()."""
        b = self.buckets.get(t_cap)
        if b is not None:
            self.buckets.move_to_end(t_cap)
            if b.grow is None:
                return b
            self.drain(b)  # a batch overflowed this bucket: drain it, widen the capacities, make it anew (b.grow: read after the drain, which may redo more)
            del self.buckets[t_cap]
            return self._add(t_cap, self.sizing.widened_caps(self.engine, b.grow, b.caps, self.batch_size * t_cap))
        if not (self.calibration and self.estimate):
            return None
        maps, n_ph_cal = self.calibration[0]  # a later bucket: capacities estimated from the phoneme count, no host round trip
        self.estimated += 1
        return self._add(t_cap, self.sizing._grown_caps(self.engine, self.sizing._ScaledMaps(maps, n_ph_cal, n_ph), self.batch_size * t_cap))

    def calibrated(self, t_cap, maps, n_ph):
        """The batch get() returned None for has run by the host route with exact maps `maps`: the first such batch is the calibration of
        every later estimate, and its bucket gets capacities from its own maps."""
        if not self.calibration:
            self.calibration.append((maps, n_ph))
        return self._add(t_cap, self.sizing._grown_caps(self.engine, maps, self.batch_size * t_cap))

    def _add(self, t_cap, caps):
        b = self.buckets[t_cap] = self.make(t_cap, caps)
        while len(self.buckets) > self.max_buckets:  # least recently used bucket out: its batches in flight are harvested first
            old_cap, old = next(iter(self.buckets.items()))
            self.drain(old)
            del self.buckets[old_cap]
            self.evicted += 1
        return b


def make_batches(lengths, batch_frames):
    """Indices sorted by length (longest first), cut into batches of at most `batch_frames` frames (at least one utterance each)."""
    order = sorted(range(len(lengths)), key=lambda i: -lengths[i])
    out, cur, tot = [], [], 0
    for i in order:
        if cur and tot + lengths[i] > batch_frames:
            out.append(cur)
            cur, tot = [], 0
        cur.append(i)
        tot += lengths[i]
    if cur:
        out.append(cur)
    return out


class Writer(object):
    """A daemon thread calling write(item) for every item put(), in order, behind a bounded queue: storage keeps up with the GPU instead of stalling
    the submit loop (file writes release the GIL).  After the first exception later items are skipped, but the event given with an item is set in
    any case, so a loop waiting for its landing buffer cannot deadlock; close() re-raises that exception on the caller's thread."""

    def __init__(self, write, maxsize):
        self._write, self._q, self._err = write, queue.Queue(maxsize=maxsize), []
        self._th = threading.Thread(target=self._run, daemon=True)
        self._th.start()

    def _run(self):
        while True:
            got = self._q.get()
            if got is None:
                return
            item, event = got
            try:
                if not self._err:
                    self._write(item)
            except Exception as e:  # surfaced by close()
                self._err.append(e)
            finally:
                if event is not None:
                    event.set()

    def put(self, item, event=None):
        self._q.put((item, event))

    def join(self):
        """Stops the thread once it has written what was put; raises nothing (for a caller with an error of its own on the way out)."""
        if self._th.is_alive():
            self._q.put(None)
            self._th.join()

    def close(self):
        self.join()
        if self._err:
            raise self._err[0]


class NullArk(object):
    """An ark sink that keeps nothing (no output prefix: synthesis and the device-to-host hand-over only)."""

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def write_batch(self, keys, mats, counts):
        pass


def chunk_selectors(plan, utts, prosody):
    """-> (spk_of, ctl_of, controlled): the speaker embeddings and the prosody controls of a chunk of `utts`, as engine.prepare / a runner's load()
    take them (None: the model has no speaker embedding / the run has no control).  prosody: None, one ProsodyControl (or its dict) for every
    utterance, or {utt_id: control} (utterances not named: None)."""
    has_spk = plan.hp.spk_embed_dim is not None
    if has_spk and any(len(u) < 3 for u in utts):
        raise ValueError("fcl-taco2_amd: the model has spk_embed_dim=%d: every utterance needs a speaker embedding" % plan.hp.spk_embed_dim)
    spk_of = (lambda chunk: [u[2] for u in chunk]) if has_spk else (lambda chunk: None)
    controlled = prosody is not None
    if isinstance(prosody, dict):  # {utt_id: control}
        per_utt = {k: ProsodyControl.coerce(v) for k, v in prosody.items()}
        ctl_of = lambda chunk: [per_utt.get(u[0]) for u in chunk]
    elif controlled:
        one = ProsodyControl.coerce(prosody)
        ctl_of = lambda chunk: [one] * len(chunk)
    else:
        ctl_of = lambda chunk: None
    return spk_of, ctl_of, controlled


def take(pending, pred=None):
    """Yields the items of the list `pending` that satisfy pred (None: all of them), removing each right before it is handed out."""
    for it in [p for p in pending if pred is None or pred(p)]:
        pending.remove(it)
        yield it
