"""fcl_taco2_amd.batching on the CPU, with fakes only: the bucket policy shared by decode.py and tts.py (calibrate once, estimate later buckets,
widen after an overflow, least recently used first out), the writer thread of the three drivers, and the selection helpers."""
import threading
import types

import numpy as np
import pytest

from fcl_taco2_amd import batching as B
from fcl_taco2_amd.prosody import ProsodyControl


class Caps(object):
    """What the policy asks of engine.Caps: it records its arguments."""

    def __init__(self, lmax, frames, bounds, tail_from=None):
        self.lmax, self.frames, self.bounds, self.tail_from = lmax, frames, np.asarray(bounds), tail_from

    def __eq__(self, other):
        return (self.lmax, self.frames, self.tail_from) == (other.lmax, other.frames, other.tail_from) and np.array_equal(self.bounds, other.bounds)


ENGINE = types.SimpleNamespace(Caps=Caps)
MAPS = types.SimpleNamespace(lmax=20, live_rows=np.arange(200, 0, -10), n_frames=900)  # the exact maps of a calibration batch


class Bucket(object):
    def __init__(self, t_cap, caps):
        self.t_cap, self.caps, self.grow = t_cap, caps, None


def store(max_buckets=8, **kw):
    log = []
    s = B.BucketStore(ENGINE, 4, Bucket, lambda b: log.append((b.t_cap, b.t_cap in s.buckets and s.buckets[b.t_cap] is b)), max_buckets, **kw)
    return s, log


def test_the_least_recently_used_bucket_is_drained_and_evicted():
    s, log = store(max_buckets=2)
    assert s.get(64, 200) is None
    a = s.calibrated(64, MAPS, 200)
    b = s.get(48, 150)
    assert s.get(64, 190) is a  # touched: B is now the oldest
    c = s.get(32, 100)
    assert list(s.buckets.items()) == [(64, a), (32, c)] and b is not c
    assert log == [(48, True)]  # drained once, while still in the mapping
    assert s.evicted == 1 and s.estimated == 2


def test_the_first_batch_calibrates_and_later_buckets_are_estimated():
    s, log = store()
    assert s.get(64, 200) is None and s.estimated == 0
    first = s.calibrated(64, MAPS, 200)
    assert first.caps == B._grown_caps(ENGINE, MAPS, 4 * 64)
    b = s.get(48, 150)
    assert isinstance(b, Bucket) and b.t_cap == 48 and s.estimated == 1
    assert b.caps == B._grown_caps(ENGINE, B._ScaledMaps(MAPS, 200, 150), 4 * 48)
    assert s.get(48, 140) is b and s.estimated == 1  # an existing bucket is used as it is
    other = types.SimpleNamespace(lmax=5, live_rows=np.full(5, 3), n_frames=10)
    s.calibrated(16, other, 7)
    assert s.calibration == [(MAPS, 200)]  # the first calibration wins
    assert s.get(32, 100).caps == B._grown_caps(ENGINE, B._ScaledMaps(MAPS, 200, 100), 4 * 32)
    assert log == [] and s.evicted == 0


def test_a_calibration_and_buckets_handed_in_are_used_and_kept():
    import collections

    buckets, cal = collections.OrderedDict(), [(MAPS, 200)]
    s, _ = store(buckets=buckets, calibration=cal)
    b = s.get(48, 150)  # no host-route batch: the calibration came with the mapping
    assert b is not None and buckets[48] is b and s.estimated == 1
    s2, _ = store(buckets=buckets, calibration=cal)
    assert s2.get(48, 150) is b and s2.estimated == 0


def test_without_estimation_every_new_length_runs_by_the_host_route():
    s, _ = store(estimate=False)
    for t_cap, n_ph in ((64, 200), (48, 150), (32, 100)):
        assert s.get(t_cap, n_ph) is None
        s.calibrated(t_cap, MAPS, n_ph)
    assert s.estimated == 0 and list(s.buckets) == [64, 48, 32] and s.get(48, 120) is s.buckets[48]


def test_an_overflowed_bucket_is_drained_and_remade_with_widened_capacities():
    s, log = store(max_buckets=1)
    s.get(64, 200)
    old = s.calibrated(64, MAPS, 200)
    old.grow = types.SimpleNamespace(lmax=3, live_rows=np.array([9, 5, 2]), n_frames=40)  # smaller than the calibration: nothing may shrink
    new = s.get(64, 180)
    assert new is not old and new.grow is None and s.buckets[64] is new and list(s.buckets) == [64]
    assert log == [(64, True)] and s.evicted == 0
    assert new.caps == B.widened_caps(ENGINE, old.grow, old.caps, 4 * 64)
    assert new.caps.lmax >= old.caps.lmax and new.caps.frames >= old.caps.frames
    assert new.caps.bounds.shape == (new.caps.lmax,) and (new.caps.bounds == 4 * 64).all()
    big = types.SimpleNamespace(lmax=100, live_rows=np.full(100, 50), n_frames=90000)
    wide = B.widened_caps(ENGINE, big, old.caps, 256)
    assert wide.lmax > old.caps.lmax and wide.frames > old.caps.frames and (wide.bounds == 256).all()


def test_the_policy_looks_the_sizing_up_on_its_module(monkeypatch):
    seen = []
    real = B._grown_caps
    monkeypatch.setattr(B, "_grown_caps", lambda eng, maps, n_rows, scale=1.3: (seen.append(scale), real(eng, maps, n_rows, scale))[1])
    scaled = []
    monkeypatch.setattr(B, "_ScaledMaps", lambda maps, a, b: (scaled.append((a, b)), MAPS)[1])
    marker = Caps(1, 1, [1])
    s, _ = store()
    s.get(64, 200)
    s.calibrated(64, MAPS, 200)
    s.get(48, 150)
    assert seen == [1.3, 1.3] and scaled == [(200, 150)]
    B.widened_caps(ENGINE, MAPS, marker, 10)
    assert seen == [1.3, 1.3, 1.6]
    monkeypatch.setattr(B, "widened_caps", lambda eng, maps, old, n_rows: marker)
    s.buckets[48].grow = MAPS
    assert s.get(48, 150).caps is marker


def test_a_module_that_reexports_the_sizing_may_be_the_place_of_substitution():
    tight = Caps(2, 256, [1, 1])
    ns = types.SimpleNamespace(_grown_caps=lambda eng, maps, n_rows, scale=1.3: tight, _ScaledMaps=B._ScaledMaps, widened_caps=B.widened_caps)
    s, _ = store(sizing=ns)
    s.get(64, 200)
    assert s.calibrated(64, MAPS, 200).caps is tight and s.get(48, 150).caps is tight
    s2, _ = store()
    s2.get(64, 200)
    assert s2.calibrated(64, MAPS, 200).caps == B._grown_caps(ENGINE, MAPS, 4 * 64)


def test_the_writer_skips_what_follows_an_error_but_sets_every_event():
    written, events = [], [threading.Event() for _ in range(3)]

    def write(item):
        if item == 1:
            raise OSError("disk full: item 1")
        written.append(item)

    w = B.Writer(write, 2)
    for i, ev in enumerate(events):
        w.put(i, ev)
    with pytest.raises(OSError, match="item 1"):
        w.close()
    assert all(ev.is_set() for ev in events) and written == [0]
    assert not w._th.is_alive()


def test_the_writer_writes_everything_in_order_before_close_returns():
    written = []
    w = B.Writer(written.append, 2)
    for i in range(20):
        w.put(i, threading.Event() if i % 2 else None)
    w.close()
    assert written == list(range(20)) and not w._th.is_alive()
    w.close()  # closing again is harmless


def test_join_stops_the_writer_without_raising_its_error():
    def write(item):
        raise OSError("writer")

    w = B.Writer(write, 2)
    w.put(0)
    w.join()  # the caller has an error of its own on the way out
    assert not w._th.is_alive()
    with pytest.raises(OSError, match="writer"):
        w.close()


def _plan(spk=None):
    return types.SimpleNamespace(hp=types.SimpleNamespace(spk_embed_dim=spk))


def test_chunk_selectors():
    utts = [("a", [1, 2]), ("b", [3]), ("c", [4, 5, 6])]
    spk_of, ctl_of, controlled = B.chunk_selectors(_plan(), utts, None)
    assert spk_of(utts) is None and ctl_of(utts) is None and controlled is False
    with pytest.raises(ValueError, match="speaker embedding"):
        B.chunk_selectors(_plan(32), utts, None)
    with_spk = [(u, x, "v" + u) for u, x in utts]
    spk_of, ctl_of, controlled = B.chunk_selectors(_plan(32), with_spk, {"a": ProsodyControl(duration_scale=2.0), "c": {"pitch_shift": 0.5}})
    assert spk_of(with_spk[1:]) == ["vb", "vc"] and controlled is True
    ctl = ctl_of(with_spk)
    assert ctl[1] is None and isinstance(ctl[0], ProsodyControl) and isinstance(ctl[2], ProsodyControl)
    assert ctl[0].duration_scale == 2.0 and ctl[2].pitch_shift == 0.5
    one = ProsodyControl(energy_scale=1.5)
    _, ctl_of, controlled = B.chunk_selectors(_plan(), utts, one)
    assert controlled is True and [c.energy_scale for c in ctl_of(utts[:2])] == [1.5, 1.5]


def test_take_removes_exactly_the_matching_items():
    pending = [1, 2, 3, 4, 5, 6]
    assert list(B.take(pending, lambda p: p % 2 == 0)) == [2, 4, 6] and pending == [1, 3, 5]
    seen = []
    for it in B.take(pending, lambda p: p > 1):
        seen.append((it, list(pending)))  # removed right before it is handed out
    assert seen == [(3, [1, 5]), (5, [1])] and pending == [1]
    assert list(B.take(pending)) == [1] and pending == []
