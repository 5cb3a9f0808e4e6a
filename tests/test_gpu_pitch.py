"""Both kernels of csrc/pitch.hip against the float64 numpy statement of tests/pitch_ref.py.  Every buffer a kernel writes sits between
guard zones filled with a NaN bit pattern, which must survive; every test reads the library's launch record and fails if its kernel did not run.
The inputs, their bounds and the conditions both have to meet are built and checked in pitch_ref.py / test_pitch_cpu.py."""
import contextlib
import functools
import json
import wave

import numpy as np
import pytest
import torch

import pitch_ref as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAT32 = 0x7FC12345  # an fp32 NaN: whatever is read from an unwritten word poisons the result
U = 2.0 ** -24


@pytest.fixture(scope="module")
def PX():
    assert torch.cuda.is_available()
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib, pitch

    _lib.load()
    return pitch


@contextlib.contextmanager
def launched(*names):
    """the launches inside run the named kernels (the library's own launch record)"""
    from fcl_taco2_amd import _lib

    _lib.prof_enable(True)
    try:
        yield
        torch.cuda.synchronize()
        seen = set(_lib.prof_collect())
    finally:
        _lib.prof_enable(False)
    for n in names:
        assert n in seen, (n, sorted(seen))


class Guarded(object):
    """a device buffer of n 32-bit words between two guard zones; everything starts as the NaN pattern"""

    PAD = 8192

    def __init__(self, *shape, dtype=torch.float32):
        self.shape, self.n = shape, int(np.prod(shape))
        self.buf = torch.empty(self.n + 2 * self.PAD, dtype=dtype, device=DEV)
        self.buf.view(torch.int32).fill_(PAT32)

    @property
    def t(self):
        return self.buf[self.PAD : self.PAD + self.n]

    def set(self, a):
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).reshape(-1))
        return self

    def np(self):
        return self.t.cpu().numpy().astype(np.float64).reshape(self.shape)

    def bits(self):
        return self.t.cpu().numpy().tobytes()

    def intact(self):
        b = self.buf.view(torch.int32)
        return bool((b[: self.PAD] == PAT32).all()) and bool((b[self.PAD + self.n :] == PAT32).all())


def plan_of(PX, geo, **kw):
    fs, hop, n, lo, hi = geo
    return PX.PitchPlan(DEV, fs=fs, hop=hop, frame_length=n, f0_floor=lo, f0_ceil=hi, **kw)


def run(PX, pl, xs, cmnd=True):
    """one px_yin_kernel launch on guarded buffers -> (maps, f0, d', tau)"""
    from fcl_taco2_amd import features

    mp = features.Maps([len(x) for x in xs], pl.hop, DEV)
    x = Guarded(sum(len(a) for a in xs)).set(np.concatenate(xs))
    f0 = Guarded(mp.frames)
    cm = Guarded(mp.frames, pl.n_lag) if cmnd else None
    tau = Guarded(mp.frames, dtype=torch.int32) if cmnd else None
    with launched("px_yin_kernel<%d>" % pl.frame_length):
        PX.launch_yin(pl, mp, x.t, f0.t, None if cm is None else cm.t, None if tau is None else tau.t)
    assert x.intact() and f0.intact() and (cm is None or (cm.intact() and tau.intact()))
    return mp, f0, cm, tau


@functools.lru_cache(maxsize=None)
def device_run(geo):
    """one launch per geometry over all its utterances, shared by the tests that compare it: host copies, read-only"""
    from fcl_taco2_amd import pitch

    ref = P.reference(geo)
    mp, f0, cm, tau = run(pitch, plan_of(pitch, geo), [x for _, x, _ in ref])
    out = dict(off=np.asarray(mp.frame_off), lens=list(mp.lens), f0=f0.np(), f0_bits=f0.bits(), dp=cm.np(), tau=tau.np().astype(np.int64))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@pytest.mark.parametrize("geo", P.GEOMETRIES, ids=str)
def test_cmnd_vs_float64(PX, geo):
    """px_yin_kernel's d'(0 .. tau_max + 1) on every utterance of the geometry against float64: per element within the derived bound
    gamma(n(tau)) d'(tau) (pitch_ref.py); wholly silent frames exactly 1 everywhere"""
    ref, dev = P.reference(geo), device_run(geo)
    assert dev["lens"] == [P.frames_of(len(x), geo[1]) for _, x, _ in ref]
    worst, silent = 0.0, 0
    for i, (name, x, r) in enumerate(ref):
        got = dev["dp"][dev["off"][i] : dev["off"][i + 1]]
        assert got.shape == r["dp"].shape and np.isfinite(got).all()
        quiet = r["energy"] == 0
        silent += int(quiet.sum())
        assert (got[quiet] == 1.0).all() and (got[:, 0] == 1.0).all()
        share = np.abs(got - r["dp"]) / r["bound"]
        worst = max(worst, float(share.max()))
        assert share.max() <= 1.0, (name, float(share.max()))
    print("pitch %r: worst share of the d' bound %.3f over %d frames (%d silent); largest bound on a frame with e(0) > 0: %.3g" %
          (geo, worst, len(dev["f0"]), silent, max(float(r["bound"][r["e0"] > 0].max()) for _, _, r in ref)))
    assert silent >= 4


@pytest.mark.parametrize("geo", P.GEOMETRIES, ids=str)
def test_pick_is_exact_on_device_cmnd(PX, geo):
    """the float64 pick run on the device's own d': tau_out and the voicing identical on EVERY frame; F0 against the float64 parabola on the same
    float32 values within (8 U (|a| + 2 |b| + |c|) / |a - 2 b + c|) / (tau + delta) + 4 U, relative"""
    fs, _, n, lo, hi = geo
    tau_min, tau_max = P.tau_range(fs, n, lo, hi)
    dev = device_run(geo)
    worst, voiced = 0.0, 0
    for f in range(len(dev["f0"])):
        dp = dev["dp"][f]
        tau, _ = P.pick(dp, tau_min, tau_max)
        assert tau == dev["tau"][f] and (dev["f0"][f] > 0) == (tau > 0), f
        if tau:
            voiced += 1
            a, b, c = dp[tau - 1], dp[tau], dp[tau + 1]
            D = a - 2.0 * b + c
            dd = min(1.0, 8.0 * U * (abs(a) + 2.0 * abs(b) + abs(c)) / abs(D)) if D != 0 else 1.0
            want = P.f0_of(dp, tau, float(fs))
            bound = dd / (fs / want - dd) + 4.0 * U
            share = abs(dev["f0"][f] / want - 1.0) / bound
            worst = max(worst, share)
            assert share <= 1.0, (f, share)
    print("pitch %r: pick identical on %d frames (%d voiced); worst share of the parabola's bound %.3f" % (geo, len(dev["f0"]), voiced, worst))
    assert voiced >= 100


@pytest.mark.parametrize("geo", P.GEOMETRIES, ids=str)
def test_f0_vs_float64(PX, geo):
    """end to end against float64: on every frame that is not fragile the same voicing and the same tau, F0 within the propagated bound
    (pitch_ref.f0_bound); fragile frames are skipped and are <= 10 % of each utterance.  The public entry adds the short-run removal."""
    ref, dev = P.reference(geo), device_run(geo)
    worst, skipped = 0.0, 0
    for i, (name, x, r) in enumerate(ref):
        a, b = dev["off"][i], dev["off"][i + 1]
        solid = ~r["fragile"]
        assert r["fragile"].sum() <= 0.1 * (b - a), name
        skipped += int(r["fragile"].sum())
        assert np.array_equal(dev["tau"][a:b][solid], r["tau"][solid]), name
        v = solid & (r["tau"] > 0)
        assert ((dev["f0"][a:b] > 0) == (dev["tau"][a:b] > 0)).all()
        if v.any():
            share = np.abs(dev["f0"][a:b][v] / r["f0"][v] - 1.0) / r["f0_bound"][v]
            worst = max(worst, float(share.max()))
            assert share.max() <= 1.0, (name, float(share.max()))
    print("pitch %r: worst share of the F0 bound %.3f; %d fragile frames skipped of %d" % (geo, worst, skipped, len(dev["f0"])))
    pt = PX.PitchTracker(plan_of(PX, geo))
    with launched("px_yin_kernel<%d>" % geo[2], "px_short_run_kernel"):
        f0, lens = pt.track_packed(np.concatenate([x for _, x, _ in ref]), [len(x) for _, x, _ in ref])
    assert lens == dev["lens"]
    want = np.concatenate([P.short_runs(dev["f0"][dev["off"][i] : dev["off"][i + 1]]) for i in range(len(ref))])
    assert np.array_equal(f0.cpu().numpy().astype(np.float64), want) and not f0.cpu().numpy()[dev["off"][-2] : dev["off"][-1]].any()  # the burst is gone


def test_short_runs(PX):
    """px_short_run_kernel: runs of 1, 2 and 3 frames at an utterance's start, end and middle, a run that would reach min_voiced only by joining the
    next utterance's, one-frame utterances; min_voiced 1 / 2 / 3 / 4: identical to the reference applied per utterance"""
    from fcl_taco2_amd import griffinlim

    V = 100.0
    utts = [[V, 0, V, V, 0, V, V, V, 0, 0, V], [V, V, 0, 0, V, V, V], [V, V, V, 0, V, V], [V, 0, V, 0, 0, V, V], [V], [0], [V, V],
            [0, V, V, V, V, 0, V, 0, 0, V, V, V]]
    rng = np.random.RandomState(3)
    utts = [np.asarray(u, dtype=np.float32) * (1.0 + rng.rand(len(u))).astype(np.float32) for u in utts]
    mp = griffinlim.Maps([len(u) for u in utts], DEV)
    flat = np.concatenate(utts)
    for mv in (1, 2, 3, 4):
        src, dst = Guarded(len(flat)).set(flat), Guarded(len(flat))
        with launched("px_short_run_kernel"):
            PX.launch_short_run(mp, src.t, dst.t, mv)
        assert src.intact() and dst.intact() and src.bits() == flat.tobytes()
        want = np.concatenate([P.short_runs(u, mv) for u in utts])
        assert dst.bits() == want.astype(np.float32).tobytes(), mv
        joined = P.short_runs(flat, mv)  # what joining runs across the borders would keep
        assert mv in (1, 4) or not np.array_equal(joined, want)


@pytest.mark.parametrize("geo", [P.GEOMETRIES[2], P.GEOMETRIES[0]], ids=str)
def test_batch_equals_per_utterance_runs_bit_for_bit(PX, geo):
    """one launch over all utterances against one launch each (another slot of the workgroup, another block: the same bits), cmnd_out / tau_out null
    against non-null, track_packed against track, and the refusal by id of a short utterance"""
    ref, dev = P.reference(geo), device_run(geo)
    xs = [x for _, x, _ in ref]
    pl = plan_of(PX, geo)
    mp, f0, cm, tau = run(PX, pl, xs)
    _, f0n, _, _ = run(PX, pl, xs, cmnd=False)
    assert f0.bits() == f0n.bits() == dev["f0_bits"]
    c, t = cm.t.reshape(mp.frames, pl.n_lag), tau.t
    for i, x in enumerate(xs):
        a, b = int(mp.frame_off[i]), int(mp.frame_off[i + 1])
        _, f1, c1, t1 = run(PX, pl, [x])
        assert f1.bits() == f0.t[a:b].cpu().numpy().tobytes() and c1.bits() == c[a:b].cpu().numpy().tobytes() and t1.bits() == t[a:b].cpu().numpy().tobytes(), i
    pt = PX.PitchTracker(pl)
    with launched("px_yin_kernel<%d>" % pl.frame_length, "px_short_run_kernel"):
        packed, lens, cm2, tau2 = pt.track_packed(np.concatenate(xs), [len(x) for x in xs], return_cmnd=True)
        each = pt.track(xs)
    assert lens == mp.lens and cm2.cpu().numpy().tobytes() == cm.bits() and tau2.cpu().numpy().tobytes() == tau.bits()
    assert torch.equal(torch.cat(each), packed)
    raw = PX.PitchTracker(plan_of(PX, geo, min_voiced=1)).track_packed(np.concatenate(xs), [len(x) for x in xs])[0]
    assert raw.cpu().numpy().tobytes() == f0.bits()  # min_voiced 1 keeps everything
    with pytest.raises(ValueError, match="utterance tiny has %d samples" % (geo[2] // 2)):
        pt.track([xs[0], xs[0][: geo[2] // 2]], ids=["ok", "tiny"])


def _write_wav(path, x, rate=22050):
    pcm = np.clip(np.rint(np.asarray(x, dtype=np.float64) * 32767.0), -32768, 32767).astype("<i2")
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(rate)
        f.writeframes(pcm.tobytes())
    return pcm.astype(np.float32) / np.float32(32768.0)


def test_driver_track_f0_end_to_end(PX, tmp_path):
    """python -m fcl_taco2_amd.extract_features --track-f0 on three generated wavs: files, shapes and dtypes; f0-ori equals phoneme_means of the
    tracker's own output bit for bit; a second run with --f0-dir on the written frame tracks gives identical f0-ori/ and f0_en_stats.npy; a manifest
    over the written files goes through train.read_train_manifest + load_batch"""
    from fcl_taco2_amd import extract_features as X, features, train

    wavs, ddir, tracks = tmp_path / "wavs", tmp_path / "dur", tmp_path / "tracks"
    wavs.mkdir()
    ddir.mkdir()
    rng = np.random.RandomState(4)
    ids, L, hz = ["ua", "ub", "uc"], [3000, 5001, 4100], [(110.0, 150.0), (240.0, 200.0), (330.0, 330.0)]
    T = [n // 256 + 1 for n in L]
    xs = {u: _write_wav(wavs / (u + ".wav"), P.harmonic(22050, np.linspace(h[0], h[1], n), rng)) for u, n, h in zip(ids, L, hz)}
    Pn = [5, 8, 6]
    for u, t, p in zip(ids, T, Pn):
        np.save(ddir / (u + ".npy"), np.full(p, t // p, dtype=np.int64))  # sums to <= T: the last entry takes the rest
    (tmp_path / "train.txt").write_text("ua\nuc\n")
    fx, pt = features.FeatureExtractor(features.FeaturePlan(DEV)), PX.PitchTracker(PX.PitchPlan(DEV))
    out1 = tmp_path / "o1"
    with launched("fx_logmel_kernel<1024>", "px_yin_kernel<1024>", "px_short_run_kernel", "fx_segment_mean_kernel"):
        got_ids, stats = X.main(["--wav-dir", str(wavs), "--feature-root", str(out1), "--durations-dir", str(ddir), "--track-f0", "--train-list",
                                 str(tmp_path / "train.txt"), "--f0-frames-out", str(tracks), "--batch-frames", "30", "--verbose", "0"])
    assert got_ids == ids and "f0" in stats
    assert sorted(p.name for p in out1.iterdir()) == ["durations_MFA", "en", "en-ori", "f0", "f0-ori", "f0_en_stats.npy", "mel_stats.npy", "mels", "mels-ori"]
    assert sorted(p.name for p in tracks.iterdir()) == [u + ".npy" for u in ids]
    fe = np.load(out1 / "f0_en_stats.npy")
    assert fe.shape == (4,) and np.log(100.0) < fe[0] < np.log(350.0) and fe[1] > 0
    for u, t, p, h in zip(ids, T, Pn, hz):
        tr, lf, d = np.load(tracks / (u + ".npy")), np.load(out1 / "f0-ori" / (u + ".npy")), np.load(out1 / "durations_MFA" / (u + ".npy"))
        assert tr.shape == (t,) and tr.dtype == np.float32 and lf.shape == (p,) and lf.dtype == np.float32 and d.sum() == t
        own = pt.track([xs[u]])[0]
        assert tr.tobytes() == own.cpu().numpy().tobytes()
        voiced = tr > 0
        assert voiced.sum() >= t // 2 and 0.9 * min(h) < np.median(tr[voiced]) < 1.1 * max(h)
        means, _ = fx.phoneme_means(X.log_f0(tr), [t], [d], mask=tr)
        assert lf.tobytes() == means.cpu().numpy().tobytes()
        fn = np.load(out1 / "f0" / (u + ".npy"))
        assert fn.shape == (p, 1) and fn.dtype == np.float32 and (fn[lf == 0, 0] == 0).all()
        assert np.allclose(fn[lf != 0, 0], (lf[lf != 0] - fe[0]) / (fe[1] + 1e-8), rtol=1e-6, atol=1e-6)

    # the written frame tracks fed back as an external tracker's
    out2 = tmp_path / "o2"
    X.main(["--wav-dir", str(wavs), "--feature-root", str(out2), "--durations-dir", str(ddir), "--f0-dir", str(tracks), "--train-list",
            str(tmp_path / "train.txt"), "--verbose", "0"])
    assert np.load(out2 / "f0_en_stats.npy").tobytes() == fe.tobytes()
    for u in ids:
        for k in ("f0-ori", "f0", "en-ori", "mels-ori"):
            assert np.load(out2 / k / (u + ".npy")).tobytes() == np.load(out1 / k / (u + ".npy")).tobytes(), (u, k)

    # a manifest over the written files is what the training driver reads
    utts = {}
    for u, t, p in zip(ids, T, Pn):
        inp = [dict(name="input%d" % (i + 1), feat=str(out1 / k / (u + ".npy")), shape=s)
               for i, (k, s) in enumerate((("mels", [t, 80]), ("durations_MFA", [p, 1]), ("f0", [p, 1]), ("en", [p, 1])))]
        utts[u] = dict(input=inp, output=[dict(name="target1", tokenid=" ".join(str(1 + (j % 40)) for j in range(p)), shape=[p, 41])])
    (tmp_path / "data.json").write_text(json.dumps({"utts": utts}))
    man = train.read_train_manifest(str(tmp_path / "data.json"))
    xs_, ys, _, ds, f0b, enb = train.load_batch(man)
    assert sorted(len(x) for x in xs_) == sorted(Pn) and [len(x) for x in xs_] == [len(d) for d in ds] == [len(f) for f in f0b] == [len(e) for e in enb]
    assert sorted(y.shape for y in ys) == sorted((t, 80) for t in T) and any(np.asarray(f).any() for f in f0b)
