"""Both kernels of csrc/pyin.hip against the numpy statement of tests/pyin_ref.py.  Every buffer a kernel writes, and the workspace, sits
between guard zones filled with a NaN bit pattern, which must survive; every test reads the library's launch record and fails if its kernel did not
run.  The float32 restatement repeats the kernels' operations in their order, so everything but the logarithm is compared bit for bit; lv and lu
are held to K_LOG ulp of the float64 logarithm (pyin_ref.py: measured once, 2.14 ulp at worst, K_LOG = 8)."""
import functools

import numpy as np
import pytest
import torch

import pitch_ref as P
import pyin_ref as Y
from test_gpu_pitch import DEV, PAT32, Guarded, _write_wav, launched, plan_of

pytestmark = pytest.mark.gpu
OBS, VIT = "pyin_obs_kernel", "pyin_viterbi_kernel"


@pytest.fixture(scope="module")
def PX():
    assert torch.cuda.is_available()
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib, pitch

    _lib.load()
    return pitch


class GuardedBytes(object):
    """the workspace: n bytes between two guard zones of the NaN pattern's words"""

    PAD = 8192

    def __init__(self, n, fill=None):
        self.n = int(n)
        self.words = -(-self.n // 4)
        self.buf = torch.empty(self.words + 2 * self.PAD, dtype=torch.int32, device=DEV)
        self.buf.fill_(PAT32)
        if fill is not None:
            self.t.fill_(fill)

    @property
    def t(self):
        return self.buf[self.PAD : self.PAD + self.words].view(torch.uint8)[: self.n]

    def intact(self):
        return bool((self.buf[: self.PAD] == PAT32).all()) and bool((self.buf[self.PAD + self.words :] == PAT32).all())


def ulps(got, want):
    """|got - want| in ulps of want's float32 binade; where want is 0 (the logarithm of a whole frame's mass, 1) got must be 0 itself"""
    zero = want == 0
    ulp = 2.0 ** (np.floor(np.log2(np.where(zero, 1.0, np.abs(want)))) - 23)
    return np.where(zero, np.where(got == 0, 0.0, np.inf), np.abs(got - want) / ulp)


# ---- launch 1 -------------------------------------------------------------------------------------------------------------------------------------
def observe(PX, pl, mp, cm):
    """one pyin_obs_kernel launch on guarded buffers -> (lv, lu, bf0, ov)"""
    lv, lu, bf0, ov = Guarded(mp.frames, pl.nb), Guarded(mp.frames), Guarded(mp.frames, pl.nb), Guarded(mp.frames, pl.nb)
    with launched(OBS):
        PX.launch_pyin_obs(pl, mp, cm, lv.t, lu.t, bf0.t, ov.t)
    assert lv.intact() and lu.intact() and bf0.intact() and ov.intact()
    return lv, lu, bf0, ov


@pytest.mark.parametrize("geo", P.GEOMETRIES, ids=str)
def test_observations_on_the_device_cmnd(PX, geo):
    """pitch_ref.utterances plus swell seed 0 through px_yin_kernel, then pyin_obs_kernel on the device's own d': ov, bf0 (hence the bins) equal the
    float32 restatement bit for bit; lv and lu within K_LOG ulp of the float64 logarithm of the device's own ov; a second launch without ov_out
    gives the same bits"""
    from fcl_taco2_amd import features

    fs, hop, n, lo, hi = geo
    tau_min, tau_max = P.tau_range(fs, n, lo, hi)
    xs = [x for _, x in P.utterances(geo)] + [Y.swell(geo, 0)]
    pl = plan_of(PX, geo, method="pyin")
    mp = features.Maps([len(x) for x in xs], hop, DEV)
    x, f0, cm = Guarded(sum(len(a) for a in xs)).set(np.concatenate(xs)), Guarded(mp.frames), Guarded(mp.frames, pl.n_lag)
    with launched("px_yin_kernel<%d>" % n):
        PX.launch_yin(pl, mp, x.t, f0.t, cm.t)
    lv, lu, bf0, ov = observe(PX, pl, mp, cm.t)
    dp = cm.t.cpu().numpy().reshape(mp.frames, pl.n_lag)
    tb = Y.geo_tables(geo, np.float32)
    assert (pl.nb, pl.band) == (tb["nb"], tb["W"])
    want = Y.observe(dp, tau_min, tau_max, tb, np.float32)
    assert ov.bits() == want["ov"].tobytes() and bf0.bits() == want["bf0"].tobytes()
    got_ov = ov.np()  # (a candidate's bin is where its mass and its F0 went: bit-equal ov and bf0 are equal bins)
    ln_v = np.log(np.maximum(got_ov, np.float64(np.float32(Y.FLOOR))))
    u = ((np.float32(1.0) - want["pv"]) / np.float32(pl.nb)).astype(np.float32)
    ln_u = np.log(np.maximum(u.astype(np.float64), np.float64(np.float32(Y.FLOOR))))
    ev, eu = ulps(lv.np(), ln_v), ulps(lu.np(), ln_u)
    print("pyin %r: %d frames, %d with several candidates; lv within %.2f ulp, lu within %.2f ulp (K_LOG %d)" %
          (geo, mp.frames, sum(len(b) > 1 for b in want["bins"]), ev.max(), eu.max(), Y.K_LOG))
    assert ev.max() <= Y.K_LOG and eu.max() <= Y.K_LOG
    assert sum(len(b) > 1 for b in want["bins"]) >= 50
    lv2, lu2, bf2 = Guarded(mp.frames, pl.nb), Guarded(mp.frames), Guarded(mp.frames, pl.nb)
    with launched(OBS):
        PX.launch_pyin_obs(pl, mp, cm.t, lv2.t, lu2.t, bf2.t)
    assert (lv2.bits(), lu2.bits(), bf2.bits()) == (lv.bits(), lu.bits(), bf0.bits()) and lv2.intact() and lu2.intact() and bf2.intact()


# ---- launch 2 -------------------------------------------------------------------------------------------------------------------------------------
class Band(object):
    """what launch_pyin_viterbi reads of a plan, for a band of any width over any number of bins"""

    def __init__(self, nb, W):
        tb = Y.band_tables(nb, W)
        self.nb, self.band, self.n_lag, self.tau_min, self.tau_max, self.fs = nb, W, 313, 27, 311, 22050.0
        self.host = tb
        self.dev_tables = {k: torch.from_numpy(np.ascontiguousarray(tb[k]).reshape(-1)).to(DEV) for k in ("tri", "la", "f_bin")}

    def workspace_bytes(self, frames):
        return frames * 2 * self.nb


def decode(PX, pl, lens, lv, lu, bf0, fill=None, utt_off=None, short=0):
    """one pyin_viterbi_kernel launch on guarded buffers over utterances of lens frames -> (state [frames], f0 bits, score [n_utt])"""
    from fcl_taco2_amd import griffinlim

    mp = griffinlim.Maps(lens, DEV)
    if utt_off is not None:
        mp.utt_off = torch.from_numpy(np.asarray(utt_off, dtype=np.int32)).to(DEV)
    glv, glu, gbf = (Guarded(*shape).set(np.array(a, dtype=np.float32)) for shape, a in (((mp.frames, pl.nb), lv), ((mp.frames,), lu), ((mp.frames, pl.nb), bf0)))
    ws = GuardedBytes(pl.workspace_bytes(mp.frames) - short, fill)
    state, f0, score = Guarded(mp.frames, dtype=torch.int32), Guarded(mp.frames), Guarded(mp.n_utt)
    with launched(VIT):
        PX.launch_pyin_viterbi(pl, mp, glv.t, glu.t, gbf.t, ws.t, state.t, f0.t, score.t)
    assert all(g.intact() for g in (glv, glu, gbf, ws, state, f0, score))
    assert glv.bits() == np.ascontiguousarray(lv, dtype=np.float32).tobytes()
    return state.t.cpu().numpy().astype(np.int64), f0.bits(), score.t.cpu().numpy()


GROUPS = sorted(set((nb, W) for nb, W, _ in Y.VITERBI_CASES))


@functools.lru_cache(maxsize=None)
def group_cases(nb, W):
    """the group's cases, noise and planted track interleaved: [(T, kind, lv, lu, bf0)]"""
    return [(T, kind) + Y.viterbi_case(nb, W, T, kind) for n, w, T in Y.VITERBI_CASES if (n, w) == (nb, W) for kind in ("noise", "track")]


@pytest.mark.parametrize("nb,W", GROUPS, ids=str)
def test_viterbi_vs_the_float32_recurrence(PX, nb, W):
    """every case of pyin_ref.VITERBI_CASES with this (nb, W), noise and planted track: all of them interleaved in ONE launch (a launch has one nb and
    one W) equal their single launches bit for bit; state and score equal the float32 recurrence bit for bit; f0 is bf0 or the bin's centre; the
    score within gamma A of the float64 sum along the device's own path and 0 <= V64 - s64(path) <= 2.1 gamma A"""
    pl, cases = Band(nb, W), group_cases(nb, W)
    lens = [c[0] for c in cases]
    state, f0, score = decode(PX, pl, lens, np.concatenate([c[2] for c in cases]), np.concatenate([c[3] for c in cases]), np.concatenate([c[4] for c in cases]))
    off = np.concatenate([[0], np.cumsum(lens)])
    for i, (T, kind, lv, lu, bf0) in enumerate(cases):
        s1, f1, v1 = decode(PX, pl, [T], lv, lu, bf0)
        assert np.array_equal(s1, state[off[i] : off[i + 1]]) and f1 == f0[4 * off[i] : 4 * off[i + 1]] and v1.tobytes() == score[i : i + 1].tobytes(), (T, kind)
        want_s, want_v, _ = Y.viterbi(lv, lu, pl.host, np.float32)
        assert np.array_equal(s1, want_s) and v1[0].tobytes() == np.float32(want_v).tobytes(), (T, kind)
        assert f1 == Y.decode_f0(want_s, bf0, pl.host).astype(np.float32).tobytes()
        if kind == "track" and T >= 6:
            assert (s1 < nb).any() and (s1 >= nb).any()  # the planted track has a voiced and an unvoiced stretch
        terms = Y.path_terms(s1, lv, lu, pl.host)
        A, g = np.abs(terms).sum(), Y.gamma_path(T)
        v64 = float(Y.viterbi(lv, lu, pl.host, np.float64)[1])
        print("pyin viterbi nb %d W %d T %d %s: |score - s64| %.3g, V64 - s64 %.3g, gamma A %.3g" % (nb, W, T, kind, abs(float(v1[0]) - terms.sum()), v64 - terms.sum(), g * A))
        assert abs(float(v1[0]) - terms.sum()) <= g * A and -1e-12 * A <= v64 - terms.sum() <= 2.1 * g * A, (T, kind)  # (the float64 sums' own rounding)


def test_viterbi_ties_equal_the_float64_path(PX):
    for name, nb, W, lv, lu in Y.tie_cases():
        pl = Band(nb, W)
        state, _, score = decode(PX, pl, [len(lv)], lv, lu, np.zeros_like(lv))
        want, v64, _ = Y.viterbi(lv, lu, pl.host, np.float64)
        assert np.array_equal(state, want) and abs(float(score[0]) - v64) <= Y.gamma_path(len(lv)) * max(abs(v64), 1.0), name


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo", P.GEOMETRIES, ids=str)
def test_swell_end_to_end(PX, geo):
    """track_packed under pyin on the swell signals (seeds 0, 1, 2) in one batch: at most 2 wrong inner frames of 54 per signal (the float64 statement
    has 0; 1 in 20 more allowed), at most 2 voiced tail frames; the same batch under yin is wrong on at least 10; the batch equals its
    per-utterance runs bit for bit; return_cmnd gives d' and the decoded states"""
    xs = [Y.swell(geo, s) for s in (0, 1, 2)]
    lens = [len(x) for x in xs]
    pt = PX.PitchTracker(plan_of(PX, geo, method="pyin"))
    with launched("px_yin_kernel<%d>" % geo[2], OBS, VIT, "px_short_run_kernel"):
        f0, flens, cm, state = pt.track_packed(np.concatenate(xs), lens, return_cmnd=True)
    assert flens == [69, 69, 69] and cm.shape == (207, pt.plan.n_lag) and state.dtype == torch.int32 and state.shape == (207,)
    got = f0.cpu().numpy().reshape(3, 69)
    st = state.cpu().numpy().reshape(3, 69)
    assert ((st >= 0) & (st < 2 * pt.plan.nb)).all() and ((got != 0) <= (st < pt.plan.nb)).all()
    yin = PX.PitchTracker(plan_of(PX, geo)).track_packed(np.concatenate(xs), lens)[0].cpu().numpy().reshape(3, 69)
    for s in range(3):
        ref = Y.swell_reference(geo, s)["f64"]["f0"]
        print("pyin %r seed %d: %d wrong inner frames (float64 %d), %d voiced tail frames; yin %d wrong" %
              (geo, s, Y.wrong_inner(got[s]), Y.wrong_inner(ref), Y.voiced_tail(got[s]), Y.wrong_inner(yin[s])))
        assert Y.wrong_inner(got[s]) <= Y.wrong_inner(ref) + 2 and Y.voiced_tail(got[s]) <= 2
        assert Y.wrong_inner(yin[s]) >= 10
        one = pt.track_packed(np.array(xs[s]), [lens[s]])[0]
        assert one.cpu().numpy().tobytes() == got[s].tobytes(), s


# ---- tables the host cannot check -------------------------------------------------------------------------------------------------------------------
def test_wild_tables_stay_inside(PX):
    """a descending and a wild utt_off, and a workspace pre-filled with 0xFF: the launch returns, the guards stay intact (decode asserts it), and the
    utterances whose slices are untouched equal the clean launch bit for bit; then the whole chain with frame_utt outside the batch"""
    from fcl_taco2_amd import features

    nb, W = 64, 5
    pl, cases = Band(nb, W), group_cases(nb, W)
    lens = [c[0] for c in cases]
    lv, lu, bf0 = (np.concatenate([c[k] for c in cases]) for k in (2, 3, 4))
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    clean = decode(PX, pl, lens, lv, lu, bf0)
    filled = decode(PX, pl, lens, lv, lu, bf0, fill=0xFF)
    assert np.array_equal(filled[0], clean[0]) and filled[1] == clean[1] and filled[2].tobytes() == clean[2].tobytes()
    for wild in ([off[0], off[1], off[2], off[1], off[4], off[5], off[6]],                      # utterance 2 descends: no frames of its own
                 [off[0], off[1], -2 ** 31, -7, off[4], off[5], off[6]],                        # 1 and 2 are empty, 3 starts at frame 0
                 [-5, off[1], off[2], off[3], off[4], off[5], 2 ** 31 - 1]):
        state, f0, score = decode(PX, pl, lens, lv, lu, bf0, utt_off=wild)
        same = [u for u in range(len(lens)) if wild[u] == off[u] and wild[u + 1] == off[u + 1]]
        overlapped = set(u for u in same for v in range(len(lens)) if v not in same and max(wild[v], 0) < off[u + 1] and min(wild[v + 1], off[-1]) > off[u])
        keep = [u for u in same if u not in overlapped]
        assert keep
        for u in keep:
            assert np.array_equal(state[off[u] : off[u + 1]], clean[0][off[u] : off[u + 1]]) and score[u : u + 1].tobytes() == clean[2][u : u + 1].tobytes(), (wild, u)
            assert f0[4 * off[u] : 4 * off[u + 1]] == clean[1][4 * off[u] : 4 * off[u + 1]]
        assert ((state[off[keep[0]] : off[keep[0] + 1]] >= 0) & (state[off[keep[0]] : off[keep[0] + 1]] < 2 * nb)).all()
    # the chain under pyin with frame_utt outside the batch: px_yin_kernel and px_short_run_kernel clamp it (here onto the frames' own utterance),
    # the new launches do not read it
    geo = P.GEOMETRIES[2]
    xs = [Y.swell(geo, 0), P.utterances(geo)[0][1]]
    pt = PX.PitchTracker(plan_of(PX, geo, method="pyin"))
    mp = features.Maps([len(x) for x in xs], geo[1], DEV)
    want = pt.track_packed(np.concatenate(xs), [len(x) for x in xs], maps=mp)[0].cpu().numpy()
    fu = mp.frame_utt.clone()
    mp.frame_utt[-3:] = 7
    mp.frame_utt[:2] = -4
    with launched(OBS, VIT):
        got = pt.track_packed(np.concatenate(xs), [len(x) for x in xs], maps=mp)[0].cpu().numpy()
    assert got.tobytes() == want.tobytes() and int((fu != mp.frame_utt).sum()) == 5


def test_refusals_launch_nothing(PX):
    """nb = 513, W = 64, W = 0 and a short workspace are refused by the entry: the launch record stays empty and no output word is written; the plan
    refuses the same by flag"""
    from fcl_taco2_amd import _lib, griffinlim

    mp = griffinlim.Maps([1], DEV)
    for nb, W, short, what in ((513, 5, 0, "nb"), (13, 64, 0, "W"), (13, 0, 0, "W"), (13, 3, 1, "workspace")):
        pl = Band(13, 3)
        pl.nb, pl.band = nb, W
        lv, lu, bf0 = Guarded(1, nb).set(np.zeros((1, nb))), Guarded(1).set(np.zeros(1)), Guarded(1, nb).set(np.zeros((1, nb)))
        ws, state, f0, score = GuardedBytes(2 * nb - short), Guarded(1, dtype=torch.int32), Guarded(1), Guarded(1)
        _lib.prof_enable(True)
        try:
            with pytest.raises(_lib.FclError, match=what):
                PX.launch_pyin_viterbi(pl, mp, lv.t, lu.t, bf0.t, ws.t, state.t, f0.t, score.t)
            torch.cuda.synchronize()
            seen = set(_lib.prof_collect())
        finally:
            _lib.prof_enable(False)
        assert VIT not in seen
        for g in (state, f0, score):
            assert bool((g.buf.view(torch.int32) == PAT32).all())
        assert bool((ws.buf == PAT32).all())
    with pytest.raises(ValueError, match="--f0-bins-per-semitone"):
        PX.PitchPlan(DEV, method="pyin", bins_per_semitone=13)
    with pytest.raises(ValueError, match="--f0-max-rate"):
        PX.PitchPlan(DEV, method="pyin", max_rate=100.0)


# ---- the driver -------------------------------------------------------------------------------------------------------------------------------------
def _tree(root):
    return {str(p.relative_to(root)): p.read_bytes() for p in sorted(root.rglob("*")) if p.is_file()}


def test_driver_f0_method(PX, tmp_path):
    """extract_features --track-f0 --f0-method pyin --f0-frames-out on three generated wavs: files, shapes and dtypes; f0-ori equals phoneme_means
    of the tracker's own output bit for bit; --f0-method yin and no method flag write byte-identical trees"""
    from fcl_taco2_amd import extract_features as X, features

    wavs, ddir = tmp_path / "wavs", tmp_path / "dur"
    wavs.mkdir()
    ddir.mkdir()
    rng = np.random.RandomState(4)
    ids, L, hz = ["ua", "ub", "uc"], [3000, 5001, 4100], [(110.0, 150.0), (240.0, 200.0), (330.0, 330.0)]
    T, Pn = [n // 256 + 1 for n in L], [5, 8, 6]
    xs = {u: _write_wav(wavs / (u + ".wav"), P.harmonic(22050, np.linspace(h[0], h[1], n), rng)) for u, n, h in zip(ids, L, hz)}
    for u, t, p in zip(ids, T, Pn):
        np.save(ddir / (u + ".npy"), np.full(p, t // p, dtype=np.int64))
    (tmp_path / "train.txt").write_text("ua\nuc\n")

    def run(name, *extra):
        out, tracks = tmp_path / name, tmp_path / (name + "_tracks")
        X.main(["--wav-dir", str(wavs), "--feature-root", str(out), "--durations-dir", str(ddir), "--track-f0", "--train-list", str(tmp_path / "train.txt"),
                "--f0-frames-out", str(tracks), "--batch-frames", "30", "--verbose", "0"] + list(extra))
        return out, tracks

    with launched("fx_logmel_kernel<1024>", "px_yin_kernel<1024>", OBS, VIT, "px_short_run_kernel", "fx_segment_mean_kernel"):
        out, tracks = run("pyin", "--f0-method", "pyin")
    assert sorted(p.name for p in out.iterdir()) == ["durations_MFA", "en", "en-ori", "f0", "f0-ori", "f0_en_stats.npy", "mel_stats.npy", "mels", "mels-ori"]
    assert sorted(p.name for p in tracks.iterdir()) == [u + ".npy" for u in ids]
    fx, pt = features.FeatureExtractor(features.FeaturePlan(DEV)), PX.PitchTracker(PX.PitchPlan(DEV, method="pyin"))
    for u, t, p, h in zip(ids, T, Pn, hz):
        tr, lf, d = np.load(tracks / (u + ".npy")), np.load(out / "f0-ori" / (u + ".npy")), np.load(out / "durations_MFA" / (u + ".npy"))
        assert tr.shape == (t,) and tr.dtype == np.float32 and lf.shape == (p,) and lf.dtype == np.float32 and d.sum() == t
        assert tr.tobytes() == pt.track([xs[u]])[0].cpu().numpy().tobytes()
        voiced = tr > 0
        assert voiced.sum() >= t // 2 and 0.9 * min(h) < np.median(tr[voiced]) < 1.1 * max(h)
        means, _ = fx.phoneme_means(X.log_f0(tr), [t], [d], mask=tr)
        assert lf.tobytes() == means.cpu().numpy().tobytes()
        assert np.load(out / "f0" / (u + ".npy")).shape == (p, 1)
    from fcl_taco2_amd import _lib

    _lib.prof_enable(True)
    try:
        a, ta = run("yin", "--f0-method", "yin")
        b, tb = run("none")
        torch.cuda.synchronize()
        seen = set(_lib.prof_collect())
    finally:
        _lib.prof_enable(False)
    assert "px_yin_kernel<1024>" in seen and OBS not in seen and VIT not in seen  # the default launches neither new kernel
    assert _tree(a) == _tree(b) and _tree(ta) == _tree(tb) and len(_tree(a)) >= 20
