"""CPU checks of the probabilistic YIN tracker: the tables, the equivalence of the candidate walk with YIN's pick run once per
threshold, the vectorised HMM against a plain triple loop, paths written by hand, the accuracy of the float64 statement of tests/pyin_ref.py on the
glide utterances and on the swell signal (where plain YIN fails), the float32 restatement against it, and the host side of the package: plan
refusals by flag, the drivers' defaults, the C entries' validation and the struct's layout, all without a GPU."""
import ctypes as C

import numpy as np
import pytest

import pitch_ref as P
import pyin_ref as Y


@pytest.fixture(scope="module")
def PX():
    from fcl_taco2_amd import pitch

    return pitch


def test_threshold_weights_and_tables(PX):
    """sum w = 1, F against a numerical integral of the Beta(2, 18) density 342 x (1 - x)^17, the bin and band counts of the four geometries, and
    the plan's tables equal to the reference's bit for bit"""
    tb = Y.geo_tables(P.GEOMETRIES[0])
    w = np.diff(tb["cw"])
    assert tb["cw"][0] == 0.0 and abs(tb["cw"][100] - 1.0) < 1e-15 and abs(w.sum() - 1.0) < 1e-15 and (w >= 0).all() and (w[:60] > 0).all()
    assert np.float32(tb["cw"][100]) == np.float32(1.0)
    x = np.linspace(0.0, 1.0, 200001)
    dens = 342.0 * x * (1.0 - x) ** 17
    integral = np.concatenate([[0.0], np.cumsum((dens[1:] + dens[:-1]) * 0.5 * (x[1] - x[0]))])
    assert np.abs(integral[::2000] - Y.beta_cdf(x[::2000])).max() < 1e-9 and abs(integral[-1] - 1.0) < 1e-9
    assert np.abs(tb["cw"] - Y.beta_cdf(np.arange(101) / 100.0)).max() < 1e-15
    assert [(Y.geo_tables(g)["nb"], Y.geo_tables(g)["W"]) for g in P.GEOMETRIES] == [(210, 25), (210, 29), (181, 25), (210, 27)]
    assert tb["tri"][25] == np.log(1.0 / 26.0) and abs(np.exp(tb["tri"]).sum() - 1.0) < 1e-12 and (np.diff(tb["edge"]) < 0).all()
    assert (np.diff(tb["edge"].astype(np.float32)) < 0).all() and (np.diff(tb["thr"]) > 0).all()
    assert tb["edge"][0] < 22050 / 71.0 and tb["edge"][-1] > 22050 / 800.0
    for geo in P.GEOMETRIES:
        fs, hop, _, lo, hi = geo
        ref, own = Y.geo_tables(geo, np.float32), PX.pyin_tables(fs, hop, lo, hi, 5, 35.92)
        assert (PX.pyin_bins(lo, hi, 5), PX.pyin_band(fs, hop, 5, 35.92)) == (ref["nb"], ref["W"])
        for k, v in own.items():
            assert v.astype(np.float32).tobytes() == ref[k].tobytes(), k


def brute_force(dp, tau_min, tau_max, tb):
    """pitch_ref.pick at each of the 100 thresholds: the mass of every threshold on the lag it picked, PA times the mass of the thresholds without a
    pick on the global minimum"""
    w = np.diff(tb["cw"])
    mass = {}
    low = tau_min + int(np.argmin(dp[tau_min : tau_max + 1]))
    for i in range(100):
        tau, _ = P.pick(dp, tau_min, tau_max, threshold=(i + 1) / 100.0)
        if tau:
            mass[tau] = mass.get(tau, 0.0) + w[i]
        else:
            mass[low] = mass.get(low, 0.0) + Y.PA * w[i]
    return mass


@pytest.mark.parametrize("geo", P.GEOMETRIES, ids=str)
def test_candidate_walk_equals_one_pick_per_threshold(geo):
    """on every frame of pitch_ref.reference(geo): the walk's candidates carry the masses of the brute force within 1e-12; lags only the walk names
    carry none (a dip no threshold separates from the record before it)"""
    fs, _, n, lo, hi = geo
    tau_min, tau_max = P.tau_range(fs, n, lo, hi)
    tb = Y.geo_tables(geo)
    frames = several = 0
    for _, _, r in P.reference(geo):
        for dp in r["dp"]:
            got = dict(Y.candidates(dp, tau_min, tau_max, tb))
            want = brute_force(dp, tau_min, tau_max, tb)
            assert set(want) <= set(got)
            for m, v in got.items():
                assert abs(v - want.get(m, 0.0)) <= 1e-12, (m, v, want.get(m))
            assert abs(sum(got.values()) - (1.0 - (1.0 - Y.PA) * tb["cw"][np.count_nonzero(tb["thr"] <= dp[tau_min : tau_max + 1].min())])) < 1e-12
            frames += 1
            several += len(want) > 1
    assert frames >= 200 and several >= 50


def test_vectorised_hmm_equals_the_triple_loop():
    for nb, W, T in ((1, 1, 3), (2, 1, 4), (7, 2, 6), (13, 20, 5), (20, 3, 9)):
        for kind in ("noise", "track"):
            lv, lu, _ = Y.viterbi_case(nb, W, T, kind)
            tb = Y.band_tables(nb, W)
            for dtype in (np.float64, np.float32):
                s1, v1, V1 = Y.viterbi(lv, lu, tb, dtype)
                s2, v2, V2 = Y.viterbi_loops(lv, lu, tb, dtype)
                assert np.array_equal(s1, s2) and v1 == v2 and V1.tobytes() == V2.tobytes() and V1.dtype == dtype


def test_paths_written_by_hand():
    """all ties; T = 1; W >= nb; a frame without candidates; digital silence"""
    for name, nb, W, lv, lu in Y.tie_cases():
        for dtype in (np.float64, np.float32):
            state, score, V = Y.viterbi(lv, lu, Y.band_tables(nb, W), dtype)
            assert (state == 0).all(), name  # the band's centre, the same voicing, the lowest index
            assert (V == V[0]).all(), name
    # T = 1: the start alone decides; the lowest index among equals
    tb = Y.band_tables(4, 2)
    lv = np.log(np.array([[0.1, 0.5, 0.5, 0.2]]))
    assert Y.viterbi(lv, np.log([0.3]), tb)[0].tolist() == [1] and Y.viterbi(lv, np.log([0.6]), tb)[0].tolist() == [4]
    # W >= nb: every bin reaches every bin; the track follows the peaks, two bins apart costs tri[W - 2]
    tb = Y.band_tables(3, 5)
    lv = np.log(np.array([[0.9, 1e-3, 1e-3], [1e-3, 1e-3, 0.9], [0.9, 1e-3, 1e-3]]))
    lu = np.log(np.full(3, 1e-4))
    state, score, _ = Y.viterbi(lv, lu, tb)
    assert state.tolist() == [0, 2, 0] and abs(score - (3 * np.log(0.9) + 2 * tb["tri"].astype(np.float64)[3] + 2 * np.log(0.99))) < 1e-6
    assert abs(Y.path_terms(state, lv, lu, tb).sum() - score) < 1e-6
    # one unvoiced frame between voiced ones is bridged or not by what it costs: ln 0.01 twice against the frame's own evidence
    tb = Y.band_tables(3, 1)
    lv = np.log(np.array([[0.9, 1e-9, 1e-9], [1e-30, 1e-30, 1e-30], [0.9, 1e-9, 1e-9]]))
    assert Y.viterbi(lv, np.log(np.array([1e-6, 0.3, 1e-6])), tb)[0].tolist() == [0, 3, 0]
    assert Y.viterbi(np.where(lv < -60, np.log(1e-3), lv), np.log(np.full(3, 0.03)), tb)[0].tolist() == [0, 0, 0]
    # a frame without candidates (every value NaN) and digital silence (d' = 1 everywhere)
    geo = P.GEOMETRIES[0]
    tau_min, tau_max = P.tau_range(geo[0], geo[2], geo[3], geo[4])
    for dtype in (np.float64, np.float32):
        tb = Y.geo_tables(geo, dtype)
        ov, bf0, pv, bins = Y.observe_frame(np.full(tau_max + 2, np.nan), tau_min, tau_max, tb, dtype)
        assert not ov.any() and not bf0.any() and pv == 0 and bins == []
        lv, lu = Y.log_obs(ov, pv, tb["nb"], dtype)
        assert np.allclose(lv, np.log(1e-30)) and np.isclose(lu, np.log(1.0 / 210))
        cand = Y.candidates(np.ones(tau_max + 2), tau_min, tau_max, tb, dtype)
        assert [m for m, _ in cand] == [tau_min] and abs(cand[0][1] - 0.01) < 1e-8  # no threshold picks: PA of the whole mass on the first lag
    # a whole utterance of zeros: the model's known weak spot.  Every frame puts PA = 0.01 on the SAME bin (that of tau_min) against
    # 0.99 / nb = 0.0047 per unvoiced bin, so the steady voiced path wins; an unvoiced run is kept only while it is shorter than what two voicing
    # switches cost (2 ln 99 / ln 2.12 = 12 frames inside an utterance).  Noise moves the bin from frame to frame and stays unvoiced (the glide tests).
    r = Y.track(np.zeros(20 * 256, dtype=np.float32), geo)
    assert (r["state"] == r["state"][0]).all() and r["state"][0] < 210 and np.allclose(r["f0"], 22050.0 / tau_min)


@pytest.mark.parametrize("geo", P.GEOMETRIES, ids=str)
def test_float64_statement_on_the_glides(geo):
    """every frame wholly inside the harmonic part voiced and within 3 % (measured: worst 1.86 %); at most 2 voiced frames among those wholly in
    noise or zeros (measured: 0 or 1)"""
    _, hop, n, _, _ = geo
    worst, inside, stray = 0.0, 0, 0
    for (name, x, r), g in zip(P.reference(geo), P.glides_of(geo)):
        assert name.startswith("glide")
        f0 = Y.track_dp(r["dp"], geo)["f0"]
        Lh = P.glide_parts(geo)[0]
        f_inst = P.glide_f_inst(geo, g)
        for t in range(len(f0)):
            a, b = t * hop - n // 2, t * hop + n // 2
            if a >= 0 and b <= Lh:
                assert f0[t] > 0, (name, t)
                worst = max(worst, abs(f0[t] / f_inst[t * hop] - 1.0))
                inside += 1
            elif a >= Lh:
                stray += int(f0[t] != 0)
    print("pyin %r: worst error %.2f %% on %d frames inside the harmonic part; %d voiced frames in noise or zeros" % (geo, 100 * worst, inside, stray))
    assert worst <= 0.03 and inside >= 100 and stray <= 2


@pytest.mark.parametrize("geo", P.GEOMETRIES, ids=str)
def test_swell_is_what_the_feature_is_for(geo):
    """seeds 0, 1, 2: the float64 statement has 0 wrong inner frames and at most 2 voiced tail frames; YIN with the short-run removal is wrong on at
    least 10 (measured: 16 or 17); the float32 restatement on float32-rounded d' agrees in voicing and in F0 within 1e-3 on >= 95 % of the frames"""
    agree = total = 0
    for seed in (0, 1, 2):
        r = Y.swell_reference(geo, seed)
        assert len(r["x"]) == 68 * geo[1] and len(r["dp"]) == 69
        assert Y.wrong_inner(r["f64"]["f0"]) == 0 and Y.voiced_tail(r["f64"]["f0"]) <= 2
        assert Y.wrong_inner(r["yin"]) >= 10
        r32 = Y.track_dp(r["dp"].astype(np.float32), geo, np.float32)
        a, b = r["f64"]["raw"], r32["raw"].astype(np.float64)
        agree += int(np.count_nonzero(((a > 0) == (b > 0)) & (np.abs(b - a) <= 1e-3 * a)))
        total += len(a)
        assert r32["raw"].dtype == np.float32 and r32["obs"]["lv"].dtype == np.float32
    print("pyin %r: float32 agrees with float64 on %d of %d frames" % (geo, agree, total))
    assert agree >= 0.95 * total


def test_bounds_of_the_viterbi_cases():
    """the GPU test's form on the float32 restatement itself, smaller cases: the score within gamma A of the float64 sum along its own path, and
    0 <= V64 - s64(path) <= 2.1 gamma A"""
    for nb, W, T in Y.VITERBI_CASES[:8]:
        for kind in ("noise", "track"):
            lv, lu, _ = Y.viterbi_case(nb, W, T, kind)
            tb = Y.band_tables(nb, W)
            s32, v32, _ = Y.viterbi(lv, lu, tb, np.float32)
            _, v64, _ = Y.viterbi(lv, lu, tb, np.float64)
            terms = Y.path_terms(s32, lv, lu, tb)
            A, g = np.abs(terms).sum(), Y.gamma_path(T)
            assert abs(float(v32) - terms.sum()) <= g * A and -1e-9 * A <= v64 - terms.sum() <= 2.1 * g * A, (nb, W, T, kind)


def test_plan_refusals_name_the_flag(PX):
    from fcl_taco2_amd import _lib

    for kw, flag in ((dict(bins_per_semitone=13), "--f0-bins-per-semitone"), (dict(bins_per_semitone=0), "--f0-bins-per-semitone"),
                     (dict(max_rate=100.0), "--f0-max-rate"), (dict(max_rate=0.5), "--f0-max-rate"), (dict(max_rate=0.0), "--f0-max-rate"),
                     (dict(hop=1024, frame_length=1024), "--f0-max-rate")):
        with pytest.raises(ValueError, match=flag):
            PX.PitchPlan("cpu", method="pyin", **kw)
        with pytest.raises(_lib.FclError, match="GPU"):
            PX.PitchPlan("cpu", **kw)  # the same numbers are not looked at under yin
    with pytest.raises(ValueError, match="--f0-method"):
        PX.PitchPlan("cpu", method="swipe")
    with pytest.raises(_lib.FclError, match="GPU"):
        PX.PitchPlan("cpu", method="pyin")  # no CPU fallback
    assert PX.pyin_bins(71.0, 800.0, 12) == 504 and PX.pyin_bins(71.0, 800.0, 13) == 546
    assert PX.pyin_band(22050, 256, 5, 35.92) == 25 and PX.pyin_band(22050, 256, 5, 90.0) == 63 and PX.pyin_band(22050, 256, 5, 92.0) == 64
    assert PX.PYIN_DEFAULTS == dict(bins_per_semitone=5, max_rate=35.92) and PX.METHODS == ("yin", "pyin")


def test_driver_defaults_are_unchanged(tmp_path):
    """every driver that shares add_pitch_arguments parses the old defaults, with --f0-method yin on top; the new flags parse and are refused by name"""
    from fcl_taco2_amd import evaluate as E, extract_features as X, preprocess as R

    wavs, durs = tmp_path / "wavs", tmp_path / "durs"
    wavs.mkdir()
    durs.mkdir()
    base = ["--wav-dir", str(wavs), "--feature-root", str(tmp_path / "out")]
    parsed = [X.parse_args(base), E.parse_args(["--ref-wav-dir", str(wavs), "--syn-wav-dir", str(wavs)]),
              R.build_parser().parse_args(["--wav-scp", "x", "--textgrid-root", "x", "--feature-root", "x"])]
    for a in parsed:
        assert (a.f0_floor, a.f0_ceil, a.f0_threshold, a.f0_min_voiced, a.f0_frame_length) == (71.0, 800.0, 0.1, 3, 1024)
        assert (a.f0_method, a.f0_bins_per_semitone, a.f0_max_rate) == ("yin", 5, 35.92)
    track = base + ["--track-f0", "--durations-dir", str(durs)]
    a = X.parse_args(track + ["--f0-method", "pyin", "--f0-bins-per-semitone", "4", "--f0-max-rate", "20"])
    assert (a.f0_method, a.f0_bins_per_semitone, a.f0_max_rate) == ("pyin", 4, 20.0)
    X.parse_args(track + ["--f0-bins-per-semitone", "13"])  # not looked at under yin
    for bad in (["--f0-method", "pyin", "--f0-bins-per-semitone", "13"], ["--f0-method", "pyin", "--f0-max-rate", "100"], ["--f0-method", "dio"]):
        with pytest.raises(SystemExit) as e:
            X.parse_args(track + bad)
        assert e.value.code == 2, bad


def test_c_entries_validate_without_a_gpu():
    from fcl_taco2_amd import _lib

    lib = _lib.load()
    assert lib.fcl_version() == _lib.ABI_VERSION == 423  # new entries and a new struct only: the revision stays
    obs, vit = lib.fcl_px_pyin_obs_fwd, lib.fcl_px_pyin_viterbi_fwd
    assert obs(None, None) == -1 and vit(None, None) == -1

    def args():
        a = _lib.Pyin()
        a.frames, a.n_utt, a.n_lag, a.tau_min, a.tau_max, a.nb, a.w, a.fs = 10, 2, 313, 27, 311, 210, 25, 22050.0
        return a

    for fn in (obs, vit):
        for nb in (0, 513, -1):
            a = args()
            a.nb = nb
            assert fn(C.byref(a), None) == -2 and b"nb" in lib.fcl_last_error()
        a = args()
        a.frames = 2 ** 31 // 420 + 1
        assert fn(C.byref(a), None) == -2 and b"2^31" in lib.fcl_last_error()
        a.frames = -1
        assert fn(C.byref(a), None) == -2
        a.frames = 0
        assert fn(C.byref(a), None) == 0  # an empty batch: nothing to launch, no pointer looked at
        assert fn(C.byref(args()), None) == -1 and b"null" in lib.fcl_last_error()
    for w in (0, 64, -3):
        a = args()
        a.w = w
        assert vit(C.byref(a), None) == -2 and b"W" in lib.fcl_last_error()
    a = args()
    a.n_utt = 65536
    assert vit(C.byref(a), None) == -2 and b"n_utt" in lib.fcl_last_error()
    a.n_utt = 0
    assert vit(C.byref(a), None) == 0
    for lo, hi, n_lag in ((1, 311, 313), (27, 512, 514), (300, 300, 313), (27, 311, 312), (27, 311, 521)):
        a = args()
        a.tau_min, a.tau_max, a.n_lag = lo, hi, n_lag
        assert obs(C.byref(a), None) == -2 and b"tau_min" in lib.fcl_last_error()
    a = args()
    a.fs = 0.0
    assert obs(C.byref(a), None) == -2 and b"fs" in lib.fcl_last_error()
    a = args()
    for k in ("lv", "lu", "bf0", "f_bin", "tri", "la", "utt_off", "workspace", "state", "f0", "score"):
        setattr(a, k, 256)
    a.workspace_bytes = 10 * 420 - 1
    assert vit(C.byref(a), None) == -5 and b"workspace" in lib.fcl_last_error()
    a.workspace = None
    a.workspace_bytes = 10 * 420
    assert vit(C.byref(a), None) == -1


def test_pyin_struct_layout_matches_the_header(tmp_path):
    import os
    import subprocess

    from conftest import ROOT
    from fcl_taco2_amd import _lib

    names = ("frames", "n_utt", "w", "fs", "cmnd", "utt_off", "ov_out", "workspace", "workspace_bytes", "state", "score")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fcl_hip.h"\nint main(void) { printf("%zu", sizeof(fcl_pyin_t));\n'
                   + "".join('printf(" %%zu", offsetof(fcl_pyin_t, %s));\n' % n for n in names) + "return 0; }\n")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")], check=True)
    out = tuple(int(v) for v in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split())
    assert out == (C.sizeof(_lib.Pyin),) + tuple(getattr(_lib.Pyin, n).offset for n in names)
