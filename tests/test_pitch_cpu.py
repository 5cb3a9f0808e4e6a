"""CPU checks of the F0 tracker: the conditions the GPU tests' own inputs (tests/pitch_ref.py) have to meet, for the reference alone
-- lengths, the size of the derived bounds, the share of fragile frames, accuracy on the harmonic part, no voicing on noise and silence, the
2-frame stretch, the mutants those bounds reject -- and the host side of the package: the tau-range refusals, the driver's new argument errors and
the C entries' validation, all without a GPU."""
import ctypes as C

import numpy as np
import pytest

import pitch_ref as P


@pytest.fixture(scope="module")
def PX():
    from fcl_taco2_amd import pitch

    return pitch


def test_geometries_and_lag_ranges(PX):
    assert [P.tau_range(fs, n, lo, hi) for fs, _, n, lo, hi in P.GEOMETRIES] == [(27, 311), (27, 311), (27, 221), (20, 226)]
    for fs, hop, n, lo, hi in P.GEOMETRIES:
        tau_min, tau_max = P.tau_range(fs, n, lo, hi)
        assert 2 <= tau_min < tau_max <= n // 2 - 1 and PX.tau_range(fs, lo, hi) == (tau_min, tau_max)
    assert [len(P.glides_of(g)) for g in P.GEOMETRIES] == [6, 6, 4, 6]


@pytest.mark.parametrize("geo", P.GEOMETRIES, ids=str)
def test_inputs_meet_their_conditions(geo):
    """every L >= N / 2 + 1 with the shortest one present and one odd frame count; the d' bound <= 1e-3 on every frame with e(0) > 0 and the form
    |delta d| <= beta (e(0) + e(tau)) no larger than 2e-4; fragile frames <= 10 % of each utterance; on frames wholly inside the harmonic part every
    frame voiced and within 3 % of the instantaneous fundamental at the frame centre; none voiced wholly inside the noise and the zeros"""
    fs, hop, n, lo, hi = geo
    ref = P.reference(geo)
    names = [name for name, _, _ in ref]
    assert names[-3:] == ["shortest", "odd", "burst"] and len(names) == len(P.glides_of(geo)) + 3
    assert P.d_beta(n) <= 2e-4
    worst_hz, worst_fragile, silent = 0.0, 0, 0
    for name, x, r in ref:
        T = P.frames_of(len(x), hop)
        assert x.dtype == np.float32 and len(x) >= n // 2 + 1 and r["dp"].shape == (T, P.tau_range(fs, n, lo, hi)[1] + 2)
        live = r["energy"] > 0  # a wholly silent frame: d' is 1 everywhere by rule
        silent += int((~live).sum())
        assert (r["bound"][r["e0"] > 0] <= 1e-3).all() and (r["bound"][r["e0"] > 0] > 0).all() and (r["dp"][:, 0] == 1).all() and (r["dp"][~live] == 1).all() and not r["tau"][~live].any()
        assert r["fragile"].sum() <= 0.1 * T, (name, int(r["fragile"].sum()), T)
        worst_fragile = max(worst_fragile, int(r["fragile"].sum()))
        voiced = r["tau"] > 0
        assert ((r["f0"] > 0) == voiced).all() and (r["f0"][voiced] >= fs / (r["tau"][voiced] + 0.5)).all()
        if name.startswith("glide"):
            g = P.glides_of(geo)[names.index(name)]
            Lh, Ln, Lz = P.glide_parts(geo)
            assert len(x) == Lh + Ln + Lz
            t = np.arange(T)
            inside = (t * hop >= n // 2) & (t * hop + n // 2 <= Lh)
            tail = (t * hop - n // 2 >= Lh) & (t * hop + n // 2 <= len(x))
            assert inside.sum() >= 30 and tail.sum() >= 10 and voiced[inside].all() and not voiced[tail].any()
            err = np.abs(r["f0"][inside] / P.glide_f_inst(geo, g)[t[inside] * hop] - 1.0)
            worst_hz = max(worst_hz, float(err.max()))
            assert err.max() <= 0.03, (name, float(err.max()))
    assert len(ref[-3][1]) == n // 2 + 1 and P.frames_of(len(ref[-2][1]), hop) % 2 == 1 and silent >= 4
    print("%r: worst F0 error on the harmonic part %.2f %%, most fragile frames in one utterance %d" % (geo, 100 * worst_hz, worst_fragile))


@pytest.mark.parametrize("geo", P.GEOMETRIES, ids=str)
def test_two_frame_stretch_and_short_runs(geo):
    """the burst utterance has exactly one voiced stretch, of 2 frames, between silences and none of its frames is fragile: it survives min_voiced 1
    and 2 and is removed at 3"""
    name, x, r = P.reference(geo)[-1]
    v = np.flatnonzero(r["tau"] > 0)
    assert name == "burst" and len(v) == 2 and v[1] == v[0] + 1 and v[0] >= 2 and v[1] <= len(r["tau"]) - 3 and not r["fragile"].any()
    assert np.array_equal(P.short_runs(r["f0"], 1), r["f0"]) and np.array_equal(P.short_runs(r["f0"], 2), r["f0"]) and not P.short_runs(r["f0"], 3).any()
    f = np.array([5.0, 0, 6, 7, 0, 1, 2, 3, 0, 9, 9])
    assert list(P.short_runs(f, 2)) == [0, 0, 6, 7, 0, 1, 2, 3, 0, 9, 9] and list(P.short_runs(f, 3)) == [0, 0, 0, 0, 0, 1, 2, 3, 0, 0, 0]
    assert list(P.short_runs(f, 4)) == [0] * 11


@pytest.mark.parametrize("geo", P.GEOMETRIES, ids=str)
def test_each_mutant_is_rejected_on_every_voiced_utterance(geo):
    """raw d in place of d', the global minimum in place of the first dip, no parabola, and W = N with wrap-around, computed in numpy on the same
    inputs: each changes the voicing, or F0 by more than 10 x the F0 bound, on at least one non-fragile frame of every utterance with voiced frames"""
    mutants = dict(raw=dict(raw=True), global_minimum=dict(first_dip=False), no_parabola=dict(interpolate=False), wrap=dict(wrap=True))
    voiced_utts = 0
    for name, x, r in P.reference(geo):
        voiced = r["tau"] > 0
        if not voiced.any():
            continue
        voiced_utts += 1
        for mname, kw in mutants.items():
            m = P.track(x, geo, **kw)
            solid = ~r["fragile"]
            flips = solid & ((m["tau"] > 0) != voiced)
            both = solid & (m["tau"] > 0) & voiced
            off = np.abs(m["f0"][both] / r["f0"][both] - 1.0) > 10.0 * r["f0_bound"][both]
            assert flips.any() or off.any(), (name, mname)
    assert voiced_utts >= len(P.glides_of(geo)) + 2


def test_reference_pick_and_parabola():
    dp = np.array([1.0, 1.0, 0.9, 0.5, 0.08, 0.05, 0.07, 0.3, 0.02, 0.6, 0.9])
    assert P.pick(dp, 2, 9) == (5, False)  # the first dip, followed downhill, not the deeper one at 8
    assert P.pick(dp, 2, 9, first_dip=False)[0] == 8 and P.pick(dp, 2, 9, threshold=0.01) == (0, False) and P.pick(dp, 6, 9)[0] == 6
    assert P.pick(dp, 2, 4)[0] == 4  # stops at tau_max
    b = np.full_like(dp, 0.006)
    assert P.pick(dp, 2, 9, bound=b) == (5, False) and P.pick(dp, 2, 9, bound=2 * b) == (5, True)  # |0.08 - 0.1| <= 2 x 0.012
    assert P.parabola(0.08, 0.05, 0.07) == pytest.approx(0.5 * 0.01 / 0.05) and P.parabola(1.0, 0.5, 0.0) == 0.0 and P.parabola(0.3, 0.1, 0.0999) == 0.5
    assert P.f0_of(dp, 5, 1000.0) == pytest.approx(1000.0 / 5.1) and P.f0_of(dp, 0, 1000.0) == 0.0 and P.f0_of(dp, 5, 1000.0, interpolate=False) == 200.0
    d = np.array([[0.0, 2.0, 4.0, 1.0], [0.0, 0.0, 0.0, 0.0]])
    assert np.allclose(P.cmnd(d), [[1.0, 1.0, 8.0 / 6.0, 3.0 / 7.0], [1.0, 1.0, 1.0, 1.0]])
    x = np.sin(np.arange(700) * 0.1)
    fr = P.frame_matrix(x, 512, 100)
    assert fr.shape == (8, 512) and fr[0, 256] == x[0] and fr[0, 255] == x[1] and fr[7, 511] == x[2 * 699 - (700 + 255)]
    assert np.allclose(P.difference(fr, 5)[:, 3], ((fr[:, :256] - fr[:, 3:259]) ** 2).sum(1)) and (P.difference(fr, 5)[:, 0] == 0).all()


def test_plan_refusals_name_the_flag(PX):
    from fcl_taco2_amd import _lib

    for kw, flag in ((dict(f0_floor=40.0), "--f0-floor"), (dict(frame_length=512), "--f0-floor"), (dict(f0_ceil=12000.0), "--f0-ceil"),
                     (dict(f0_floor=500.0, f0_ceil=400.0), "--f0-ceil"), (dict(threshold=0.0), "--f0-threshold"), (dict(min_voiced=0), "--f0-min-voiced"),
                     (dict(fs=48000), "--f0-floor")):
        with pytest.raises(ValueError, match=flag):
            PX.PitchPlan("cpu", **kw)
    for kw, flag in ((dict(frame_length=2048), "--f0-frame-length"), (dict(hop=0), "--hop")):
        with pytest.raises(NotImplementedError, match=flag):
            PX.PitchPlan("cpu", **kw)
    with pytest.raises(_lib.FclError, match="GPU"):
        PX.PitchPlan("cpu")  # no CPU fallback
    assert PX.DEFAULTS == dict(fs=22050, hop=256, frame_length=1024, f0_floor=71.0, f0_ceil=800.0, threshold=0.1, min_voiced=3)
    assert PX.tau_range(22050, 71.0, 800.0) == (27, 311)


def test_driver_argument_errors(tmp_path):
    from fcl_taco2_amd import extract_features as X

    wavs, durs = tmp_path / "wavs", tmp_path / "durs"
    wavs.mkdir()
    durs.mkdir()
    base = ["--wav-dir", str(wavs), "--feature-root", str(tmp_path / "out")]
    a = X.parse_args(base)
    assert not a.track_f0 and a.f0_frames_out is None
    assert (a.f0_floor, a.f0_ceil, a.f0_threshold, a.f0_min_voiced, a.f0_frame_length) == (71.0, 800.0, 0.1, 3, 1024)
    a = X.parse_args(base + ["--track-f0", "--durations-dir", str(durs), "--f0-frames-out", str(tmp_path / "tracks"), "--f0-floor", "100", "--f0-frame-length", "512"])
    assert a.track_f0 and (a.f0_floor, a.f0_frame_length, a.f0_frames_out) == (100.0, 512, str(tmp_path / "tracks"))
    X.parse_args(base + ["--f0-floor", "40"])  # without --track-f0 the range is not looked at: the driver behaves as before
    for bad, what in ((base + ["--track-f0", "--durations-dir", str(durs), "--f0-dir", str(durs)], "mutually exclusive"),
                      (base + ["--track-f0"], "--track-f0 needs --durations-dir"),
                      (base + ["--track-f0", "--durations-dir", str(durs), "--f0-floor", "40"], "--f0-floor 40 Hz is too low"),
                      (base + ["--track-f0", "--durations-dir", str(durs), "--f0-frame-length", "512"], "--f0-floor 71 Hz is too low"),
                      (base + ["--track-f0", "--durations-dir", str(durs), "--f0-ceil", "20000"], "--f0-ceil"),
                      (base + ["--track-f0", "--durations-dir", str(durs), "--f0-frame-length", "768"], "--f0-frame-length"),
                      (base + ["--track-f0", "--durations-dir", str(durs), "--f0-min-voiced", "0"], "--f0-min-voiced"),
                      (base + ["--f0-frames-out", str(tmp_path / "tracks")], "--f0-frames-out needs --track-f0")):
        with pytest.raises(SystemExit) as e:
            X.parse_args(bad)
        assert e.value.code == 2, bad


def test_c_entries_validate_without_a_gpu():
    from fcl_taco2_amd import _lib

    lib = _lib.load()
    assert lib.fcl_version() == _lib.ABI_VERSION  # new entries and a new struct only: the revision stays
    fn = lib.fcl_px_yin_fwd
    assert fn(None, None) == -1
    a = _lib.Pitch()
    a.n, a.hop, a.tau_min, a.tau_max, a.frames, a.n_utt, a.samples, a.fs, a.threshold = 768, 256, 27, 311, 10, 1, 5000, 22050.0, 0.1
    assert fn(C.byref(a), None) == -2 and b"n must be 512 or 1024" in lib.fcl_last_error()
    a.n, a.hop = 1024, 0
    assert fn(C.byref(a), None) == -2 and b"hop" in lib.fcl_last_error()
    for lo, hi in ((1, 311), (27, 512), (300, 300)):
        a.hop, a.tau_min, a.tau_max = 256, lo, hi
        assert fn(C.byref(a), None) == -2 and b"tau_min" in lib.fcl_last_error()
    a.tau_min, a.tau_max, a.n = 27, 311, 512
    assert fn(C.byref(a), None) == -2 and b"tau_max 311, n 512" in lib.fcl_last_error()
    a.n, a.threshold = 1024, 0.0
    assert fn(C.byref(a), None) == -2 and b"threshold" in lib.fcl_last_error()
    a.threshold, a.n_utt = 0.1, 11
    assert fn(C.byref(a), None) == -2 and b"n_utt" in lib.fcl_last_error()
    a.n_utt, a.frames = 2, 2 ** 31 // 313 + 1
    assert fn(C.byref(a), None) == -2 and b"2^31" in lib.fcl_last_error()
    a.frames, a.samples = 10, 2 ** 31
    assert fn(C.byref(a), None) == -2 and b"samples" in lib.fcl_last_error()
    a.samples = 5000
    assert fn(C.byref(a), None) == -1 and b"null x" in lib.fcl_last_error()
    a.x = a.smp_off = a.frame_utt = a.utt_off = 256
    assert fn(C.byref(a), None) == -1 and b"null f0" in lib.fcl_last_error()
    sr = lib.fcl_px_short_run_fwd
    assert sr(None, None, None, None, 10, 1, 3, None) == -1 and b"null" in lib.fcl_last_error()
    assert sr(256, 256, 256, 256, 10, 1, 3, None) == -1 and b"must not be f0_in" in lib.fcl_last_error()
    assert sr(256, 256, 256, 512, 1, 2, 3, None) == -2 and b"frames >= n_utt" in lib.fcl_last_error()
    assert sr(256, 256, 256, 512, 2 ** 31, 2, 3, None) == -2
    assert sr(256, 256, 256, 512, 10, 1, 0, None) == -2 and b"min_voiced" in lib.fcl_last_error()


def test_pitch_struct_layout_matches_the_header(tmp_path):
    import os
    import subprocess

    from conftest import ROOT
    from fcl_taco2_amd import _lib

    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fcl_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(fcl_px_t), '
                   'offsetof(fcl_px_t, tau_max), offsetof(fcl_px_t, fs), offsetof(fcl_px_t, x), offsetof(fcl_px_t, tau_out)); return 0; }\n')
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")], check=True)
    out = tuple(int(v) for v in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split())
    assert out == (C.sizeof(_lib.Pitch), _lib.Pitch.tau_max.offset, _lib.Pitch.fs.offset, _lib.Pitch.x.offset, _lib.Pitch.tau_out.offset)
