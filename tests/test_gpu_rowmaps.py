"""-m gpu: the integer row / frame maps built ON THE DEVICE (fcl_row_maps_build) are bit-identical to the host maps (engine.build_row_maps, itself
pinned to the reference's converter / inference bookkeeping by G4), and a synthesis pass driven by them — forced or PREDICTED durations, eager or
as a replayed hipGraph — equals the pass with host-built maps.  Reference: ..._kd_student.py:821-851, decoder_sa_kd.py:736-791 (H10); a predicted
duration of 0 is the reference's AssertionError (decoder_sa_kd.py:739) and must surface here as FCL_STATUS_ZERO_DURATION."""
import os

import numpy as np
import pytest
import torch

from helpers import max_abs, np_state_dict
from fcl_taco2_amd import hparams as HP, synthetic as SYN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _dev_maps(lens, durs, lmax_cap, frames_cap, mode):
    """mode "compact": rows = the non-padded phonemes (row_src / utt_row0 from the lengths); "padded": rows = the padded [B, T] layout."""
    from fcl_taco2_amd import ops

    B, T = len(lens), max(lens)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    if mode == "compact":
        starts = np.concatenate([[0], np.cumsum(lens)])
        row_src = np.concatenate([b * T + np.arange(n) for b, n in enumerate(lens)])
        d = np.concatenate([np.asarray(x).reshape(-1) for x in durs])
        out = ops.row_maps_build(int(starts[-1]), B, lmax_cap, frames_cap, dur_i32=i32(d), row_src=i32(row_src), utt_row0=i32(starts), want_order=True, status=st)
    else:
        dpad = np.zeros((B, T), dtype=np.int64)
        pad = np.ones((B, T), dtype=np.uint8)
        for b, n in enumerate(lens):
            dpad[b, :n] = np.asarray(durs[b]).reshape(-1)
            pad[b, :n] = 0
        out = ops.row_maps_build(B * T, B, lmax_cap, frames_cap, dur_i64=torch.from_numpy(dpad.reshape(-1)).to(DEV), t_max=T,
                                 pad=torch.from_numpy(pad.reshape(-1)).to(DEV), want_order=True, status=st)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, int(st.item()) & 0xFFFFFFFF


def _check_equal(lens, durs, slack_l=0, slack_f=0):
    from fcl_taco2_amd import engine

    m = engine.build_row_maps(lens, durs, max(lens))
    n = len(m.src_rows)
    for mode in ("compact", "padded"):
        d, status = _dev_maps(lens, durs, m.lmax + slack_l, m.n_frames + slack_f, mode)
        assert status == 0, (mode, status)
        assert np.array_equal(d["src_rows"][:n], m.src_rows) and np.array_equal(d["dur"][:n], m.dur_sorted), mode
        assert np.array_equal(d["frame_off"][:n], m.frame_off_sorted), mode
        assert np.array_equal(d["live_rows"][: m.lmax], m.live_rows) and not d["live_rows"][m.lmax :].any(), mode
        assert np.array_equal(d["frame_lo"][: m.n_frames], m.frame_lo) and np.array_equal(d["frame_hi"][: m.n_frames], m.frame_hi), mode
        assert not d["frame_lo"][m.n_frames :].any() and not d["frame_hi"][m.n_frames :].any(), mode
        assert list(np.diff(d["utt_frame0"])) == m.utt_frames and tuple(d["totals"][:3]) == (m.n_frames, m.lmax, 0), mode
        if mode == "compact":
            assert np.array_equal(d["order"], m.order)
        else:  # padding rows sort behind every real row, carry duration 0 and the total as their frame offset
            assert not d["dur"][n:].any() and (d["frame_off"][n:] <= m.n_frames).all()


def test_device_row_maps_equal_host_maps_on_g4_and_fuzz():
    g = dict(np.load(os.path.join(GOLDEN, "g4_integer.npz")))
    ds = [g["in_ds%d" % i].reshape(-1).astype(np.int64) for i in range(4)]
    ds = [np.maximum(d, 1) for d in ds]  # (the converter's batch has zero-duration phonemes: inference would assert on them, see below)
    _check_equal([len(d) for d in ds], ds)
    rng = np.random.RandomState(0)
    cases = [([1], [[1]]), ([1], [[50]]), ([3, 1], [[2, 2, 2], [2]]), ([5, 5], [[1, 1, 1, 1, 1], [7, 7, 7, 7, 7]])]
    for trial in range(40):
        B = int(rng.randint(1, 40))
        lens = sorted(rng.randint(1, 130, size=B).tolist(), reverse=True)
        hi = int(rng.choice([2, 5, 50, 300]))
        cases.append((lens, [rng.randint(1, hi + 1, size=n) for n in lens]))
    xs, c2 = SYN.batch_c2(80, batch=64, seed=11)  # the configs[4] batch: 5 k rows, > one LDS chunk of the builder
    cases.append(([len(d) for d in c2], c2))
    for i, (lens, durs) in enumerate(cases):
        _check_equal(lens, durs, slack_l=(i % 3) * 5, slack_f=(i % 4) * 100)


def test_device_row_maps_report_violations_and_decode_nothing():
    from fcl_taco2_amd import _lib

    lens, durs = [4, 3], [[3, 0, 2, 1], [1, 1, 9]]
    d, status = _dev_maps(lens, durs, 16, 64, "padded")
    assert status == _lib.STATUS_ZERO_DURATION and not d["live_rows"].any() and d["totals"][2] == 1  # the reference's AssertionError (D9)
    durs = [[3, 1, 2, 1], [1, 1, 9]]
    for mode in ("compact", "padded"):
        d, status = _dev_maps(lens, durs, 8, 64, mode)  # max duration 9 > 8 launched steps
        assert status == _lib.STATUS_LMAX_CAP and not d["live_rows"].any() and not d["frame_hi"].any()
        d, status = _dev_maps(lens, durs, 9, 17, mode)  # 18 frames > 17
        assert status == _lib.STATUS_FRAMES_CAP and not d["live_rows"].any()
        d, status = _dev_maps(lens, durs, 9, 18, mode)
        assert status == 0 and d["live_rows"][0] == 7 and d["totals"][0] == 18


def test_row_maps_built_inside_the_bilstm_launch_equal_the_standalone_builder():
    """fcl_bilstm_fwd(row_maps=...): H = 128 builds the maps in one extra workgroup of the persistent recurrence, every other width with the
    builder's own launches after it: identical tensors and status bits, and the recurrence's output is unchanged."""
    from fcl_taco2_amd import _lib, ops

    rng = np.random.RandomState(5)
    for h, c, lens, hi in [(128, 64, [37, 30, 9, 1], 12), (128, 32, sorted(rng.randint(1, 120, size=33).tolist(), reverse=True), 40),
                           (64, 32, [21, 20, 3], 6), (128, 32, [5, 4], 0)]:
        B, T = len(lens), max(lens)
        dpad = np.zeros((B, T), dtype=np.int32)
        pad = np.ones((B, T), dtype=np.uint8)
        for b, n in enumerate(lens):
            dpad[b, :n] = rng.randint(1, hi + 1, size=n) if hi else 0  # hi = 0: every duration zero (the reference's AssertionError)
            pad[b, :n] = 0
        lmax, frames = int(max(dpad.max(), 1)) + 3, int(dpad.sum()) + 50
        g = torch.Generator().manual_seed(h + B)
        w = [(0.2 * torch.randn(sh, generator=g)).to(DEV) for sh in [(4 * h, c), (4 * h, h), (4 * h,), (4 * h, c), (4 * h, h), (4 * h,)]]
        x = torch.randn(B * T, c, generator=g).to(DEV)
        lens_dev = torch.tensor(lens, dtype=torch.int32, device=DEV)
        d_dev, pad_dev = torch.from_numpy(dpad.reshape(-1)).to(DEV), torch.from_numpy(pad.reshape(-1)).to(DEV)
        st_a, st_b = (torch.zeros(1, dtype=torch.int32, device=DEV) for _ in range(2))
        alone = ops.row_maps_build(B * T, B, lmax, frames, dur_i32=d_dev, t_max=T, pad=pad_dev, want_order=True, status=st_a)
        req = ops.row_maps_request(B * T, B, lmax, frames, dur_i32=d_dev, t_max=T, pad=pad_dev, want_order=True, status=st_b)
        for v in req.maps.values():
            v.fill_(-7)
        out = ops.bilstm(x, lens_dev, *w, B, T, row_maps=req)
        ref = ops.bilstm(x, lens_dev, *w, B, T)
        torch.cuda.synchronize()
        assert torch.equal(out, ref)
        assert int(st_a.item()) == int(st_b.item()) == (0 if hi else _lib.STATUS_ZERO_DURATION)
        for k in alone:
            if k != "scratch":
                assert torch.equal(alone[k], req.maps[k]), (h, k)


def _plan(hp, sd=None):
    from fcl_taco2_amd.plan import SynthesisPlan

    return SynthesisPlan(sd if sd is not None else np_state_dict(hp), hp, DEV)


def test_forced_durations_through_device_maps_equal_host_maps():
    """The same batch, forced durations: host-built maps vs device-built maps with exact capacities (same kernels per step -> bit-identical) and with
    generous ones (every step may keep every row: other tile shapes -> fp32 summation order)."""
    from fcl_taco2_amd import engine, ops

    hp = HP.student_hparams(dropout_rate=0.0)
    plan = _plan(hp)
    xs, ds = SYN.batch_c2(hp.idim, batch=12, t_lo=40, t_hi=90, seed=21)
    ref = torch.cat(engine.synthesize(plan, xs, ds))
    maps = engine.build_row_maps([len(x) for x in xs], ds, max(len(x) for x in xs))
    n_pad = len(xs) * max(len(x) for x in xs)
    exact = torch.cat(engine.synthesize(plan, xs, ds, caps=engine.Caps.from_maps(maps)))
    assert torch.equal(exact, ref)
    gen = torch.cat(engine.synthesize(plan, xs, ds, caps=engine.Caps.generous(n_pad, maps.lmax + 7, maps.n_frames + 1000)))
    assert gen.shape == ref.shape and max_abs(gen, ref) < 2e-5
    ops.check_status(DEV)
    # a step bound below the device's count is flagged, not silently wrong
    tight = engine.Caps.from_maps(maps)
    tight.bounds[3] -= 1
    with pytest.raises(Exception, match="live rows"):
        engine.synthesize(plan, xs, ds, caps=tight)
    # a zero duration is the reference's AssertionError on either path
    bad = [d.copy() for d in ds]
    bad[1][2] = 0
    with pytest.raises(AssertionError):
        engine.synthesize(plan, xs, bad)
    with pytest.raises(Exception, match="zero duration"):
        engine.synthesize(plan, xs, bad, caps=engine.Caps.from_maps(maps))


def test_predicted_durations_without_a_host_round_trip_and_as_a_graph():
    """Predicted durations (the reference's inference() default): predictor -> clamp(round(exp(x) - 1), 0) -> row maps, all in HBM.  The eager pass
    with the host round trip is the reference behaviour; the device-driven pass and a replayed hipGraph of it must give the same mel."""
    from fcl_taco2_amd import engine, ops

    hp = HP.student_hparams(dropout_rate=0.0)
    plan = _plan(hp, SYN.positive_duration_head(np_state_dict(hp)))
    xs, _ = SYN.batch_c2(hp.idim, batch=8, t_lo=30, t_hi=70, seed=33)
    prep = engine.prepare(plan, xs)
    mel_ref, frames_ref, inter = engine.run(plan, prep, return_intermediates=True)
    torch.cuda.synchronize()
    m = inter["maps"]
    assert min(m.utt_frames) > 0 and 3 <= m.lmax <= 64 and m.dur_sorted.min() >= 1  # the synthetic duration head predicts usable durations
    n_pad = prep.B * prep.T
    mel_dev, frames = engine.run(plan, prep, caps=engine.Caps.generous(n_pad, m.lmax + 9, m.n_frames + 777))
    assert frames.resolve() == list(m.utt_frames)
    assert max_abs(mel_dev[: m.n_frames], mel_ref) < 2e-5
    runner = engine.GraphRunner(plan, prep)  # calibrates, then captures predictor + rounding + device maps + decoder + postnet
    for _ in range(3):
        out = runner.replay()
        torch.cuda.synchronize()
        runner.check()
        assert torch.equal(out[: m.n_frames], mel_ref) and runner.utt_frames == list(m.utt_frames)
    assert np.array_equal(np.diff(runner.frames.utt_frame0.cpu().numpy()), np.asarray(m.utt_frames))
    # other ids through the SAME graph would need other capacities: a violated capacity is reported, never silent
    small = engine.Caps(2, 64, np.full(2, n_pad, dtype=np.int32))
    engine.run(plan, prep, caps=small)
    with pytest.raises(Exception, match="decoder steps|frames"):
        ops.check_status(DEV)


def test_batch_runner_one_graph_for_many_batches():
    """engine.BatchRunner: ONE captured graph, capacities instead of a baked-in batch.  Different batches (other lengths, other durations, fewer
    utterances than the capacity) go through load() + replay() and must equal the plain eager synthesis of each batch; a batch that does not fit
    is reported."""
    from fcl_taco2_amd import engine

    hp = HP.student_hparams(dropout_rate=0.0)
    plan = _plan(hp)
    B, T_cap = 8, 64
    batches = [SYN.batch_c2(hp.idim, batch=B, t_lo=20, t_hi=T_cap, seed=s) for s in (1, 2, 3)]
    batches.append(tuple(v[:5] for v in SYN.batch_c2(hp.idim, batch=B, t_lo=10, t_hi=30, seed=4)))  # fewer utterances than the capacity
    maps = [engine.build_row_maps([len(x) for x in xs], ds, T_cap) for xs, ds in batches]
    lmax = max(m.lmax for m in maps) + 2
    bounds = np.zeros(lmax, dtype=np.int32)
    for m in maps:
        bounds[: m.lmax] = np.maximum(bounds[: m.lmax], m.live_rows)
    bounds = np.maximum(bounds, 1)
    caps = engine.Caps(lmax, max(m.n_frames for m in maps) + 100, bounds)
    runner = engine.BatchRunner(plan, B, T_cap, caps, forced=True)
    for (xs, ds), m in zip(batches + batches[:1], maps + maps[:1]):  # (and the first batch again: nothing of the previous one may linger)
        runner.load(xs, ds)
        mel = runner.replay()
        assert runner.frames() == list(m.utt_frames)
        ref = torch.cat(engine.synthesize(plan, xs, ds))
        assert max_abs(mel[: m.n_frames], ref) < 2e-5
    xs, ds = batches[0]
    bad = [d.copy() for d in ds]
    bad[0][0] = lmax + 1
    runner.load(xs, bad)
    runner.replay()
    with pytest.raises(Exception, match="decoder steps"):
        runner.frames()
    with pytest.raises(ValueError):
        runner.load(xs + xs, ds + ds)
    # predicted durations through one graph
    plan2 = _plan(hp, SYN.positive_duration_head(np_state_dict(hp)))
    r2 = engine.BatchRunner(plan2, B, T_cap, engine.Caps.generous(B * T_cap, 64, B * T_cap * 24), forced=False)
    for xs, _ in batches[:2]:
        r2.load(xs)
        mel = r2.replay()
        fr = r2.frames()
        ref = engine.synthesize(plan2, xs)
        assert fr == [int(m_.shape[0]) for m_ in ref] and max_abs(mel[: sum(fr)], torch.cat(ref)) < 2e-5


def test_the_in_graph_feed_equals_the_copy_in_front_of_the_launch(monkeypatch):
    """BatchRunner's input block: pulled out of pinned host memory by the graph's first node (fcl_feed_copy, the default) or copied by one
    hipMemcpyAsync in front of every launch (FCL_FEED_INGRAPH=0): the same mels bit for bit, batch after batch, also when the host repacks the
    block right after a launch (it must wait for the feed node's sequence number) and when a pass is replayed without a new load."""
    from fcl_taco2_amd import engine

    hp = HP.student_hparams(dropout_rate=0.0)
    plan = _plan(hp)
    B, T_cap = 6, 48
    batches = [SYN.batch_c2(hp.idim, batch=B, t_lo=12, t_hi=T_cap, seed=s) for s in (11, 12, 13, 14)]
    maps = [engine.build_row_maps([len(x) for x in xs], ds, T_cap) for xs, ds in batches]
    caps = engine.Caps.generous(B * T_cap, max(m.lmax for m in maps) + 1, max(m.n_frames for m in maps) + 64)
    outs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("FCL_FEED_INGRAPH", mode)
        r = engine.BatchRunner(plan, B, T_cap, caps, forced=True)
        assert r._ingraph == (mode == "1")
        res = []
        for i in range(12):  # back to back: the host is ahead of the device, every load() finds the previous pass still queued
            xs, ds = batches[i % 4]
            r.load(xs, ds)
            with torch.cuda.stream(r.stream):  # (the copy is ordered behind the pass on the runner's stream: no host synchronisation in the loop)
                res.append(r.replay().clone())
        with torch.cuda.stream(r.stream):
            res.append(r.replay().clone())  # the same block again
        assert r.frames() == list(maps[11 % 4].utt_frames)
        outs[mode] = res
    for a, b in zip(outs["1"], outs["0"]):
        assert torch.equal(a, b)
    for i, m in enumerate(maps):
        ref = torch.cat(engine.synthesize(plan, *batches[i]))
        assert max_abs(outs["1"][i][: m.n_frames], ref) < 2e-5
    assert torch.equal(outs["1"][12][: maps[3].n_frames], outs["1"][11][: maps[3].n_frames])


def test_decode_driver_recovers_from_a_capacity_overflow(tmp_path, monkeypatch):
    """fcl_taco2_amd.decode: a batch that exceeds its bucket's calibrated capacities is reported by the device, re-run on the host-mapped path and the
    bucket's graphs are re-captured with larger capacities; every utterance's mel still equals the plain synthesis.  Forced here by shrinking the
    calibration (half the frames, two thirds of the steps of the calibrating batch)."""
    from fcl_taco2_amd import decode as D, engine
    from fcl_taco2_amd.kaldi_io import read_scp

    S, T = HP.student_hparams(dropout_rate=0.0), HP.teacher_hparams()
    model = SYN.build_model("student", S, T, DEV).eval()
    sd = SYN.positive_duration_head(SYN.closed_form_state_dict(HP.param_spec(S, T, True)))
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    model = model.to(DEV).eval()
    rng = np.random.RandomState(4)
    utts = [("u%03d" % i, rng.randint(1, S.idim, size=int(rng.randint(40, 48))).astype(np.int64)) for i in range(40)]  # one bucket (48), 5 batches of 8

    def tight(eng, maps, n_rows, scale=1.3):
        lmax = max(2, (2 * maps.lmax) // 3)
        return eng.Caps(lmax, max(256, maps.n_frames // 2), np.full(lmax, n_rows, dtype=np.int32))

    real = D._grown_caps
    calls = []
    monkeypatch.setattr(D, "_grown_caps", lambda eng, maps, n_rows, scale=1.3: (calls.append(scale), tight(eng, maps, n_rows) if len(calls) == 1 else real(eng, maps, n_rows, scale))[1])
    st = {}
    frames, _ = D.decode(model, utts, str(tmp_path / "f"), batch_size=8, depth=2, stats=st)
    assert st["redone_batches"] >= 1 and st["eager_batches"] == 1 and st["graph_batches"] >= 3
    mels = read_scp(str(tmp_path / "f.scp"))
    assert sorted(mels) == sorted(u for u, _ in utts) and frames == sum(m.shape[0] for m in mels.values())
    plan = model.plan()
    for uid, x in utts[::7]:
        ref = engine.synthesize(plan, [x])[0]
        assert mels[uid].shape == tuple(ref.shape) and max_abs(mels[uid], ref) < 2e-5


def test_decode_driver_estimates_later_buckets_capacities_from_phoneme_counts(tmp_path, monkeypatch):
    """Round 6: only the FIRST bucket of a corpus is calibrated by an eager batch; the capacities of later buckets are the calibrated maps
    rescaled by phoneme count (decode._ScaledMaps) + the usual slack.  Three length buckets: one eager batch, two estimated buckets, every mel equal to plain
    synthesis; an estimate that is too tight (forced: frames / 3) is caught by the device and recovered like any overflow."""
    from fcl_taco2_amd import decode as D, engine
    from fcl_taco2_amd.kaldi_io import read_scp

    S, T = HP.student_hparams(dropout_rate=0.0), HP.teacher_hparams()
    model = SYN.build_model("student", S, T, DEV).eval()
    sd = SYN.positive_duration_head(SYN.closed_form_state_dict(HP.param_spec(S, T, True)))
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    model = model.to(DEV).eval()
    rng = np.random.RandomState(9)
    utts = [("u%03d" % i, rng.randint(1, S.idim, size=int(n)).astype(np.int64)) for i, n in enumerate(list(rng.randint(50, 64, 16)) + list(rng.randint(34, 48, 16)) +
                                                                                                      list(rng.randint(18, 32, 16)))]
    st = {}
    frames, _ = D.decode(model, utts, str(tmp_path / "e"), batch_size=8, depth=2, stats=st)
    assert st["eager_batches"] == 1 and st["estimated_buckets"] == 2 and st["buckets"] == 3 and st["redone_batches"] == 0, st
    mels = read_scp(str(tmp_path / "e.scp"))
    assert sorted(mels) == sorted(u for u, _ in utts) and frames == sum(m.shape[0] for m in mels.values())
    plan = model.plan()
    for uid, x in utts[::5]:
        ref = engine.synthesize(plan, [x])[0]
        assert mels[uid].shape == tuple(ref.shape) and max_abs(mels[uid], ref) < 2e-5
    # an estimate that does not hold: the device reports it, the batch is redone on the host-mapped path, the bucket grows
    D.release_graphs(model)
    real = D._ScaledMaps

    class Tight(real):
        def __init__(self, maps, n_ph_cal, n_ph):
            real.__init__(self, maps, n_ph_cal, n_ph)
            self.n_frames = max(64, self.n_frames // 3)

    monkeypatch.setattr(D, "_ScaledMaps", Tight)
    st2 = {}
    frames2, _ = D.decode(model, utts, str(tmp_path / "t"), batch_size=8, depth=2, stats=st2)
    assert st2["estimated_buckets"] == 2 and st2["redone_batches"] >= 1 and frames2 == frames, st2
    mels2 = read_scp(str(tmp_path / "t.scp"))
    for uid, _ in utts[::5]:
        assert max_abs(mels2[uid], mels[uid]) < 2e-5


def test_decode_driver_evicts_least_recently_used_buckets(tmp_path):
    """max_buckets=1 with three length buckets: every new bucket evicts the one before it -- its batch in flight is harvested and its pinned landing
    buffers are waited for first -- and no utterance is lost or altered on the way.  The calibration stays with the plan: a second call on the same
    model estimates every bucket and runs no eager batch."""
    from fcl_taco2_amd import decode as D, engine
    from fcl_taco2_amd.kaldi_io import read_scp

    S, T = HP.student_hparams(dropout_rate=0.0), HP.teacher_hparams()
    model = SYN.build_model("student", S, T, DEV).eval()
    sd = SYN.positive_duration_head(SYN.closed_form_state_dict(HP.param_spec(S, T, True)))
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    model = model.to(DEV).eval()
    rng = np.random.RandomState(9)
    utts = [("u%03d" % i, rng.randint(1, S.idim, size=int(n)).astype(np.int64)) for i, n in enumerate(list(rng.randint(50, 64, 8)) + list(rng.randint(34, 48, 8)) +
                                                                                                      list(rng.randint(18, 32, 8)))]
    st = {}
    frames, _ = D.decode(model, utts, str(tmp_path / "v"), batch_size=4, depth=2, stats=st, max_buckets=1)
    assert st["eager_batches"] == 1 and st["estimated_buckets"] == 2 and st["evicted_buckets"] == 2 and st["buckets"] == 1 and st["redone_batches"] == 0, st
    mels = read_scp(str(tmp_path / "v.scp"))
    assert sorted(mels) == sorted(u for u, _ in utts) and frames == sum(m.shape[0] for m in mels.values())
    plan = model.plan()
    for uid, x in utts[::5]:
        ref = engine.synthesize(plan, [x])[0]
        assert mels[uid].shape == tuple(ref.shape) and max_abs(mels[uid], ref) < 2e-5
    st2 = {}
    frames2, _ = D.decode(model, utts, str(tmp_path / "w"), batch_size=4, depth=2, stats=st2, max_buckets=1)
    assert st2["eager_batches"] == 0 and frames2 == frames, st2


def test_grouped_predictor_launches_equal_the_per_predictor_path():
    """plan.PredictorGroup: the duration / pitch / energy predictors (one geometry in the shipped recipes) as ONE launch per layer -- a Conv1d with
    the stacked output channels, grouped LayerNorms, a grouped Conv1d, grouped LayerNorm + head -- against one launch per predictor and layer:
    same outputs (the stacked layer-0 GEMM and the grouped kernels compute every output element exactly as the separate ones do)."""
    from fcl_taco2_amd import engine, ops

    if not ops.planes_enabled():
        pytest.skip("FCL_PRECISION=0: the grouped launches exist on the pre-split operand path only")
    hp = HP.student_hparams(dropout_rate=0.0)
    plan = _plan(hp, SYN.positive_duration_head(np_state_dict(hp)))
    assert plan.group_pe is not None and plan.group_dpe is not None and plan.group_dpe.G == 3
    xs, _ = SYN.batch_c2(hp.idim, batch=6, t_lo=30, t_hi=70, seed=5)
    prep = engine.prepare(plan, xs)
    hs, hs_p = engine.encode(plan, prep, planes=True)
    m = prep.B * prep.T
    d, p, e = engine._predictors_grouped(plan.group_dpe, hs_p, prep.seg_lo, prep.seg_hi, prep.pad, m, [True, True, True])
    p2, e2 = engine._predictors_grouped(plan.group_pe, hs_p, prep.seg_lo, prep.seg_hi, prep.pad, m, [True, True])
    for got, pp in ((d, plan.duration), (p, plan.pitch), (e, plan.energy), (p2, plan.pitch), (e2, plan.energy)):
        ref = engine._predictor_scalar_planes(pp, hs_p, prep.seg_lo, prep.seg_hi, prep.pad)
        assert got.shape == ref.shape and max_abs(got, ref) < 1e-6 * max(1.0, float(ref.abs().max()))
    # and end to end: the pass with grouped predictors (default) against the reference-pinned oracle path is covered by the mel tests; here
    # grouped vs ungrouped synthesis of the same batch
    mel_g, fr, _ = engine.run(plan, prep, return_intermediates=True)
    engine._GROUP_PREDICTORS = False
    try:
        mel_u, fr_u, _ = engine.run(plan, prep, return_intermediates=True)
    finally:
        engine._GROUP_PREDICTORS = True
    assert list(fr) == list(fr_u) and max_abs(mel_g, mel_u) < 1e-5


def test_decode_driver_and_capacity_graphs_carry_speaker_embeddings(tmp_path):
    """spk_embed_dim through the capacity-graph feed: the speaker vectors of a batch travel in the runner's input block (one H2D copy), the graph
    appends F.normalize(spemb) to the encoder states (fcl_concat_spk_fwd); the decode driver reads (utt_id, ids, spemb) and every mel equals the
    eager synthesis of that utterance with its own speaker; a speaker-embedding model without vectors is refused."""
    from fcl_taco2_amd import decode as D, engine
    from fcl_taco2_amd.kaldi_io import read_scp

    S, T = HP.student_hparams(dropout_rate=0.0, spk_embed_dim=32), HP.teacher_hparams()
    import argparse
    from fcl_taco2_amd.nets.knowledge_distillation.e2e_tts_tacotron2_sa_kd_student import Tacotron2_sa as Student

    ns = lambda h: argparse.Namespace(embed_dim=h.embed_dim, eunits=h.eunits, econv_chans=h.econv_chans, dunits=h.dunits, prenet_units=h.prenet_units,
                                      postnet_chans=h.postnet_chans, use_residual=False, use_masking=True, dropout_rate=h.dropout_rate,
                                      duration_predictor_chans=h.duration_predictor_chans, spk_embed_dim=h.spk_embed_dim)
    com = argparse.Namespace(use_fe_condition=True, append_position=True, distill_output_knowledge=True, distill_encoder_knowledge=True,
                             distill_decoder_knowledge=True, distill_prosody_knowledge=True, is_train=False, share_proj=True)
    model = Student(S.idim, S.odim, ns(S), com, ns(T))
    spec = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    sd = SYN.positive_duration_head(SYN.closed_form_state_dict(spec))
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    model = model.to(DEV).eval()
    rng = np.random.RandomState(9)
    utts = [("s%03d" % i, rng.randint(1, S.idim, size=int(rng.randint(20, 32))).astype(np.int64), rng.randn(32).astype(np.float32)) for i in range(24)]
    st = {}
    frames, _ = D.decode(model, utts, str(tmp_path / "g"), batch_size=8, depth=2, stats=st)
    assert st["graph_batches"] >= 1
    mels = read_scp(str(tmp_path / "g.scp"))
    assert sorted(mels) == sorted(u[0] for u in utts) and frames == sum(m.shape[0] for m in mels.values())
    plan = model.plan()
    for uid, x, sp in utts[::5]:
        ref = engine.synthesize(plan, [x], spembs=[sp])[0]
        other = engine.synthesize(plan, [x], spembs=[-sp])[0]
        assert mels[uid].shape == tuple(ref.shape) and max_abs(mels[uid], ref) < 2e-5
        assert other.shape != ref.shape or max_abs(other, ref) > 1e-3  # the speaker vector matters
    with pytest.raises(ValueError):
        D.decode(model, [(u, x) for u, x, _ in utts], None, batch_size=8)
