"""Compact phoneme rows on the CPU: the block BatchRunner.load() packs for a row capacity (engine.Caps.rows) against the padded [batch, t_cap] block of
the same batch, field by field, and the row capacities Caps.for_batches / batching._grown_caps hand out.  The runner here is the host side only
(BatchRunner._host_init without pinned memory): no device call is made."""
import numpy as np
import pytest

from fcl_taco2_amd import batching, engine
from fcl_taco2_amd import prosody as P

B, T = 4, 12


def host_runner(rows, monkeypatch, forced=True, controls=False):
    monkeypatch.delenv("FCL_FEED_INGRAPH", raising=False)  # the in-graph feed: load() is host packing only
    r = object.__new__(engine.BatchRunner)
    r.B, r.T, r.S, r.forced, r.controls = B, T, 0, forced, controls
    r._host_init(rows, 1, pin=False)
    return r


def fields(r):
    hb = r._host[0].numpy()
    seg = lambda name, dt: hb[r._off[name][0] : r._off[name][0] + r._off[name][1]].view(dt)
    out = dict(ids=seg("ids", np.int64), lo=seg("seg_lo", np.int32), hi=seg("seg_hi", np.int32), dur=seg("dur", np.int32), lens=seg("lens", np.int32)[:B],
               pad=seg("pad", np.uint8))
    if r.controls:
        out["ctl"] = seg("ctl", np.float32).reshape(-1, P.NCTL)
    if r.R is not None:
        out["row0"], out["total"] = seg("row0", np.int32)[: B + 1], int(seg("row0", np.int32)[B + 1])
    return out


def batch(lens, seed=0):
    g = np.random.default_rng(seed)
    return [g.integers(1, 40, n).astype(np.int64) for n in lens], [g.integers(1, 9, n).astype(np.int64) for n in lens]


def check_against_padded(c, p, lens, rows):
    nb, total = len(lens), int(sum(lens))
    valid = p["pad"] == 0
    assert int(valid.sum()) == total and c["ids"].shape[0] == rows and p["ids"].shape[0] == B * T
    starts = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    # the real rows: the padded block's valid rows, in order
    assert np.array_equal(c["ids"][:total], p["ids"][valid]) and np.array_equal(c["dur"][:total], p["dur"][valid])
    assert not c["pad"][:total].any()
    b_of = np.repeat(np.arange(nb), lens)
    assert np.array_equal(c["lo"][:total], starts[b_of]) and np.array_equal(c["hi"][:total], starts[b_of + 1])
    assert np.array_equal(p["lo"][valid], b_of * T)  # the same segment, relative to the utterance's first row
    assert np.array_equal(c["hi"][:total] - c["lo"][:total], p["hi"][valid] - p["lo"][valid])
    # the rows behind the total: PAD id, empty segment, duration 0, pad = 1
    assert not c["ids"][total:].any() and not c["dur"][total:].any() and (c["pad"][total:] == 1).all()
    assert np.array_equal(c["lo"][total:], c["hi"][total:])
    # lengths and row ranges
    assert np.array_equal(c["lens"], p["lens"]) and np.array_equal(c["lens"][:nb], lens) and not c["lens"][nb:].any()
    assert np.array_equal(c["row0"][: nb + 1], starts) and (c["row0"][nb:] == total).all() and c["total"] == total


@pytest.mark.parametrize("lens,rows", [((1, T, 7), 24), ((1, T, 7), 20), ((T, T, T, T - 1), 47), ((3,), 4)])
def test_compact_block_against_the_padded_block(lens, rows, monkeypatch):
    xs, ds = batch(lens)
    rp, rc = host_runner(None, monkeypatch), host_runner(rows, monkeypatch)
    stale_x, stale_d = batch((5, 5, 5, 4), seed=9)  # a fuller batch first: nothing of it may survive the second load
    for r in (rp, rc):
        if sum(len(x) for x in stale_x) <= (r.R or B * T):
            r.load(stale_x, stale_d)
        r.load(xs, ds)
    assert rc.R == rows and rp.R is None and rc.n_loaded == len(lens)
    check_against_padded(fields(rc), fields(rp), np.asarray(lens), rows)


def test_total_equal_to_the_capacity_fits_and_one_more_row_is_refused(monkeypatch):
    lens = (1, T, 7)
    xs, ds = batch(lens)
    r = host_runner(sum(lens), monkeypatch)
    r.load(xs, ds)
    f = fields(r)
    assert f["total"] == sum(lens) == r.R and not f["pad"].any()
    before = r._host[0].numpy().copy()
    xs2, ds2 = batch((2, T, 7), seed=3)
    with pytest.raises(ValueError, match="row capacity"):
        r.load(xs2, ds2)
    assert np.array_equal(r._host[0].numpy(), before) and r.n_loaded == 3  # the previous block stays intact


def test_prosody_rows_follow_the_phonemes(monkeypatch):
    lens = (1, T, 7)
    xs, _ = batch(lens)
    g = np.random.default_rng(4)
    ctl = [P.ProsodyControl(pitch_scale=g.uniform(0.5, 2.0, n), energy_shift=g.uniform(-1, 1, n)) for n in lens]
    rp, rc = host_runner(None, monkeypatch, forced=False, controls=True), host_runner(24, monkeypatch, forced=False, controls=True)
    rp.load(xs, prosody=ctl)
    rc.load(xs, prosody=ctl)
    p, c = fields(rp), fields(rc)
    total = sum(lens)
    assert c["ctl"].shape == (24, P.NCTL) and np.array_equal(c["ctl"][:total], p["ctl"][p["pad"] == 0])
    assert (c["ctl"][total:] == np.asarray(P.IDENTITY, np.float32)).all()
    rc.load(xs)  # no controls: identity everywhere
    assert (fields(rc)["ctl"] == np.asarray(P.IDENTITY, np.float32)).all()


def test_row_capacities_of_for_batches_and_grown_caps():
    sets = [batch((5, 9, 2)), batch((7, 7, 8), seed=1), batch((1, 1, 3), seed=2)]
    maps = [engine.build_row_maps([len(x) for x in xs], ds, T) for xs, ds in sets]
    assert engine.Caps.for_batches(maps).rows == 22  # the largest phoneme-row count of the batches
    assert engine.Caps.from_maps(maps[0]).rows is None and engine.Caps.generous(B * T, 8, 512).rows is None  # the padded universe
    assert engine.Caps(4, 256, np.ones(4, np.int32), rows=17).rows == 17
    m = maps[1]  # 22 phoneme rows
    g = batching._grown_caps(engine, m, 3 * T)
    assert g.rows == g.bounds[0] == min(3 * T, int(22 * 1.3) + 32)  # the live rows' slack, capped at the padded universe
    assert batching._grown_caps(engine, m, 1000).rows == int(22 * 1.3) + 32
    assert batching.widened_caps(engine, m, g, 3 * T).rows is None  # after an overflow: every row, the padded layout
    scaled = batching._grown_caps(engine, batching._ScaledMaps(m, 22, 11), 1000)
    assert scaled.rows == int(np.ceil(m.live_rows[0] * 0.5) * 1.3) + 32
