"""Both kernels of csrc/features.hip against the float64 numpy statement of tests/features_ref.py.  Every buffer a kernel writes sits
between guard zones filled with a NaN bit pattern, which must survive; every test reads the library's launch record and fails if its kernel did not
run.  The inputs, their bounds and the conditions both have to meet are built and checked in features_ref.py / test_features_cpu.py."""
import contextlib
import functools
import json
import wave

import numpy as np
import pytest
import torch

import features_ref as F
import griffinlim_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAT32 = 0x7FC12345  # an fp32 NaN: whatever is read from an unwritten word poisons the result
U = 2.0 ** -24


@pytest.fixture(scope="module")
def FX():
    assert torch.cuda.is_available()
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib, features

    _lib.load()
    return features


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
    """a float32 device buffer of n words between two guard zones; everything starts as the NaN pattern"""

    PAD = 8192

    def __init__(self, *shape):
        self.shape, self.n = shape, int(np.prod(shape))
        self.buf = torch.empty(self.n + 2 * self.PAD, dtype=torch.float32, device=DEV)
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


def plan_of(FX, case, **kw):
    n_fft, hop, wl = case
    return FX.FeaturePlan(DEV, n_fft=n_fft, hop=hop, win_length=wl, **kw)


@functools.lru_cache(maxsize=None)
def reference(case):
    """computed once per case and shared: the inputs, and per utterance (S, E, log-mel) in float64 with the three bounds"""
    n_fft, hop, _ = case
    xs, B, w = F.signals(case), F.filterbank(case), R.hann_window(case[2], case[0])
    per = [F.features(x.astype(np.float64), w, hop, B) for x in xs]
    S, E, lm = (np.concatenate([p[i] for p in per]) for i in range(3))
    for a in (S, E, lm):
        a.setflags(write=False)
    return dict(xs=xs, B=B, S=S, E=E, lm=lm, b_mag=F.magnitude_bound(S, n_fft), b_en=F.energy_bound(S, n_fft), b_mel=F.logmel_bound(S, B, n_fft))


def run(FX, pl, xs, mag=True, stats=True):
    mp = FX.Maps([len(x) for x in xs], pl.hop, DEV)
    x = Guarded(sum(len(a) for a in xs)).set(np.concatenate(xs))
    mel, en = Guarded(mp.frames, pl.A), Guarded(mp.frames)
    mg = Guarded(mp.frames, pl.bins) if mag else None
    with launched("fx_logmel_kernel<%d>" % pl.n_fft):
        FX.launch_logmel(pl, mp, x.t, mel.t, en.t, None if mg is None else mg.t, stats=stats)
    assert x.intact() and mel.intact() and en.intact() and (mg is None or mg.intact())
    return mp, mel, en, mg


@pytest.mark.parametrize("case", F.CASES, ids=str)
def test_magnitudes_energy_and_logmel_vs_float64(FX, case):
    """fx_logmel_kernel on four utterances (the shortest allowed length, lengths hop does not divide, one with wholly silent frames) against float64:
    per frame ||S_gpu - S||_2 <= fb ||C||_2, |dE| <= (fb + 4 U) E, per element |d log10| <= dM / (M ln 10) + 4 U max(1, |log10 M|) (features_ref.py;
    fb = Higham's norm-form FFT bound).  Silent frames: log-mel within the bound of -10, energy exactly 0."""
    ref = reference(case)
    pl = plan_of(FX, case)
    assert np.allclose(FX.dense_filterbank(pl.fb_lo, pl.fb_off, pl.fb_w, pl.bins), ref["B"], rtol=1e-12, atol=1e-15)  # the package builds the same matrix
    mp, mel, en, mg = run(FX, pl, ref["xs"])
    assert mp.lens == [F.frames_of(len(x), case[1]) for x in ref["xs"]] and mp.frames == len(ref["E"])
    S, E, lm = mg.np(), en.np(), mel.np()
    assert np.isfinite(S).all() and np.isfinite(E).all() and np.isfinite(lm).all()
    silent = ref["E"] == 0
    live = ~silent
    r_mag = np.linalg.norm(S - ref["S"], axis=1)[live] / ref["b_mag"][live]
    r_en = np.abs(E - ref["E"])[live] / ref["b_en"][live]
    r_mel = np.abs(lm - ref["lm"]) / ref["b_mel"]
    print("features %r: worst share of the bound: magnitudes %.3f, energy %.3f, log-mel %.3f (silent frames %.3f); largest log-mel bound %.3g" %
          (case, r_mag.max(), r_en.max(), r_mel[live].max(), r_mel[silent].max(), ref["b_mel"].max()))
    assert r_mag.max() <= 1.0 and r_en.max() <= 1.0 and r_mel.max() <= 1.0
    assert silent.sum() >= 2 and (E[silent] == 0).all() and (S[silent] == 0).all() and (ref["lm"][silent] == -10.0).all()


@pytest.mark.parametrize("case", F.CASES, ids=str)
def test_normalised_logmel_vs_float64(FX, case):
    """the same with mel_stats: (v - mean) / (std + 1e-8) against float64 on the float32 statistics, the log-mel bound divided by (std + 1e-8)"""
    ref = reference(case)
    stats = F.stats_case().astype(np.float32)
    pl = plan_of(FX, case, mel_stats=stats)
    assert np.array_equal(pl.stats_d.cpu().numpy(), stats)
    _, mel, en, _ = run(FX, pl, ref["xs"], mag=False)
    s64 = stats.astype(np.float64)
    want = (ref["lm"] - s64[0]) / (s64[1] + 1e-8)
    ratio = np.abs(mel.np() - want) / (ref["b_mel"] / (s64[1] + 1e-8))
    print("normalised features %r: worst share of the bound %.3f" % (case, ratio.max()))
    assert np.isfinite(mel.np()).all() and ratio.max() <= 1.0
    assert (np.abs(en.np() - ref["E"]) <= ref["b_en"]).all()
    _, raw, _, _ = run(FX, pl, ref["xs"], mag=False, stats=False)  # the plan's statistics left out: the unnormalised rows
    assert (np.abs(raw.np() - ref["lm"]) <= ref["b_mel"]).all()


@pytest.mark.parametrize("case", [(512, 100, 512), (1024, 256, 1024), (2048, 300, 2048)], ids=str)
def test_batch_equals_per_utterance_runs_bit_for_bit(FX, case):
    """one launch over four utterances against four launches of one (another slot of the workgroup, another block: the same bits), and mag_out null
    against non-null"""
    ref = reference(case)
    pl = plan_of(FX, case)
    mp, mel, en, mg = run(FX, pl, ref["xs"])
    _, mel0, en0, _ = run(FX, pl, ref["xs"], mag=False)
    assert mel.bits() == mel0.bits() and en.bits() == en0.bits()
    m, e, g = mel.t.reshape(mp.frames, pl.A), en.t, mg.t.reshape(mp.frames, pl.bins)
    for i, x in enumerate(ref["xs"]):
        a, b = int(mp.frame_off[i]), int(mp.frame_off[i + 1])
        _, mel1, en1, mg1 = run(FX, pl, [x])
        assert mel1.bits() == m[a:b].cpu().numpy().tobytes() and en1.bits() == e[a:b].cpu().numpy().tobytes() and mg1.bits() == g[a:b].cpu().numpy().tobytes(), i
    # the public entries on the same samples
    fx = FX.FeatureExtractor(pl)
    with launched("fx_logmel_kernel<%d>" % pl.n_fft):
        rows, energy, lens, mags = fx.extract_packed(np.concatenate(ref["xs"]), [len(x) for x in ref["xs"]], return_magnitudes=True)
        each = fx.extract(ref["xs"])
    assert lens == mp.lens and rows.cpu().numpy().tobytes() == mel.bits() and energy.cpu().numpy().tobytes() == en.bits() and mags.cpu().numpy().tobytes() == mg.bits()
    assert torch.equal(torch.cat([m_ for m_, _ in each]), rows) and torch.equal(torch.cat([e_ for _, e_ in each]), energy)
    loud = [3.0 * ref["xs"][1]]  # a peak above 1: divided by the peak first
    assert float(np.abs(loud[0]).max()) > 1.0
    assert torch.equal(fx.extract(loud)[0][0], fx.extract([loud[0] / np.float32(np.abs(loud[0]).max())])[0][0])
    with pytest.raises(ValueError, match="utterance tiny has %d samples" % (case[0] // 2)):
        fx.extract([ref["xs"][0], ref["xs"][0][: case[0] // 2]], ids=["ok", "tiny"])


def test_segment_means_vs_numpy(FX):
    """fx_segment_mean_kernel on random durations with zero-length phonemes, a one-phoneme utterance and, in the nonzero_only form, a phoneme whose
    frames are all unvoiced: per segment |d mean| <= (n + 2) U mean|v| over the n entries that count; an empty set gives exactly 0"""
    rng = np.random.RandomState(11)
    durs = [rng.randint(0, 9, size=23), np.array([17]), rng.randint(0, 5, size=300), np.array([0, 0, 6, 0])]
    durs[0][[2, 7]] = 0
    T = [int(d.sum()) for d in durs]
    v = (rng.randn(sum(T)) * 3.0 + 5.0).astype(np.float32)
    mask = (rng.rand(sum(T)) < 0.6).astype(np.float32) * v
    a0 = int(durs[0][:4].sum())
    assert durs[0][4] > 0
    mask[a0 : a0 + int(durs[0][4])] = 0.0  # phoneme 4 of utterance 0: all unvoiced
    n_ph = [len(d) for d in durs]
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)
    args = (i32(np.concatenate(durs)), i32(np.repeat(np.arange(4), n_ph)), i32(np.concatenate([[0], np.cumsum(n_ph)])), i32(np.concatenate([[0], np.cumsum(T)])))
    fo = np.concatenate([[0], np.cumsum(T)])
    for use_mask in (False, True):
        vd, md, out = Guarded(len(v)).set(v), Guarded(len(v)).set(mask), Guarded(sum(n_ph))
        with launched("fx_segment_mean_kernel"):
            FX.launch_segment_mean(vd.t, md.t if use_mask else None, *args, out.t, 4, use_mask)
        assert out.intact() and vd.intact() and md.intact()
        got, worst, k, empties = out.np(), 0.0, 0, 0
        for u, d in enumerate(durs):
            vu, mu = v[fo[u] : fo[u + 1]].astype(np.float64), mask[fo[u] : fo[u + 1]]
            want = F.segment_means(vu, d, mu if use_mask else None)
            a = 0
            for p, n in enumerate(d):
                seg = vu[a : a + n][mu[a : a + n] != 0] if use_mask else vu[a : a + n]
                if len(seg) == 0:
                    assert got[k] == 0.0
                    empties += 1
                else:
                    worst = max(worst, abs(got[k] - want[p]) / ((len(seg) + 2) * U * np.abs(seg).mean()))
                a, k = a + n, k + 1
        print("segment means (nonzero_only=%s): worst share of the bound %.3f, %d empty segments" % (use_mask, worst, empties))
        assert worst <= 1.0 and empties >= 5 and (not use_mask or got[4] == 0.0)
    # the public entry adjusts each utterance's last duration by T - sum(durations) first
    fx = FX.FeatureExtractor(plan_of(FX, (1024, 256, 1024)))
    short = [d.copy() for d in durs]
    short[0][-1] += 3
    short[2][-1] = 0
    with launched("fx_segment_mean_kernel"):
        means, adj = fx.phoneme_means(v, T, short)
    assert all(int(d.sum()) == t for d, t in zip(adj, T))
    want = np.concatenate([F.segment_means(v[fo[u] : fo[u + 1]], adj[u]) for u in range(4)])
    assert np.abs(means.cpu().numpy() - want).max() <= 12 * U * np.abs(v).max()
    with pytest.raises(ValueError, match="utterance #1 has 17 frames"):
        fx.phoneme_means(v, T, [durs[0], np.array([18, 2]), durs[2], durs[3]])


def _write_wav(path, x, rate=22050):
    pcm = np.clip(np.rint(np.asarray(x, dtype=np.float64) * 32767.0), -32768, 32767).astype("<i2")
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(rate)
        f.writeframes(pcm.tobytes())
    return pcm.astype(np.float32) / np.float32(32768.0)


def test_driver_end_to_end(FX, tmp_path):
    """python -m fcl_taco2_amd.extract_features on three tiny wavs: files, shapes and dtypes; mels-ori equals extract() on the same samples; with
    --train-list the normalised mels have per-channel mean 0 and standard deviation 1 over the listed utterances within 1e-5, and a manifest that
    points at the written files goes through train.read_train_manifest + load_batch"""
    from fcl_taco2_amd import extract_features as X, train

    wavs, ddir, fdir = tmp_path / "wavs", tmp_path / "dur", tmp_path / "f0"
    for d in (wavs, ddir, fdir):
        d.mkdir()
    rng = np.random.RandomState(2)
    ids, L = ["ua", "ub", "uc"], [3000, 5001, 4100]
    T = [n // 256 + 1 for n in L]
    xs = {u: _write_wav(wavs / (u + ".wav"), 0.8 * R.signal(30 + i, n)) for i, (u, n) in enumerate(zip(ids, L))}
    P = [5, 8, 6]
    durs, f0s = {}, {}
    for u, t, p in zip(ids, T, P):
        d = np.full(p, t // p, dtype=np.int64)  # sums to <= T: the last entry takes the rest
        durs[u] = d
        np.save(ddir / (u + ".npy"), d)
        f = (120.0 + 40.0 * rng.rand(t + 2)) * (rng.rand(t + 2) < 0.7)  # two frames more than T: truncated
        f[: d[0]] = 0.0  # the first phoneme: all unvoiced
        f0s[u] = f
        np.save(fdir / (u + ".npy"), f)
    (tmp_path / "train.txt").write_text("ua\nuc\n")
    fx = FX.FeatureExtractor(FX.FeaturePlan(DEV))
    want = {u: fx.extract([xs[u]])[0] for u in ids}

    # frame-level run: no durations, no statistics
    out1 = tmp_path / "o1"
    with launched("fx_logmel_kernel<1024>"):
        got_ids, stats = X.main(["--wav-dir", str(wavs), "--feature-root", str(out1), "--batch-frames", "30", "--verbose", "0"])
    assert got_ids == ids and stats is None and sorted(p.name for p in out1.iterdir()) == ["en-ori", "mels-ori"]
    for u, t in zip(ids, T):
        m, e = np.load(out1 / "mels-ori" / (u + ".npy")), np.load(out1 / "en-ori" / (u + ".npy"))
        assert m.shape == (t, 80) and m.dtype == np.float32 and e.shape == (t,) and e.dtype == np.float32
        assert m.tobytes() == want[u][0].cpu().numpy().tobytes() and e.tobytes() == want[u][1].cpu().numpy().tobytes()

    # the full run
    out2 = tmp_path / "o2"
    (tmp_path / "wav.scp").write_text("".join("%s %s\n" % (u, wavs / (u + ".wav")) for u in ids))
    with launched("fx_logmel_kernel<1024>", "fx_segment_mean_kernel"):
        _, stats = X.main(["--wav-scp", str(tmp_path / "wav.scp"), "--feature-root", str(out2), "--durations-dir", str(ddir), "--f0-dir", str(fdir),
                           "--train-list", str(tmp_path / "train.txt"), "--verbose", "0"])
    assert sorted(p.name for p in out2.iterdir()) == ["durations_MFA", "en", "en-ori", "f0", "f0-ori", "f0_en_stats.npy", "mel_stats.npy", "mels", "mels-ori"]
    mel_stats, fe = np.load(out2 / "mel_stats.npy"), np.load(out2 / "f0_en_stats.npy")
    assert mel_stats.shape == (2, 80) and fe.shape == (4,) and (mel_stats[1] > 0).all() and fe[1] > 0 and fe[3] > 0
    for u, t, p in zip(ids, T, P):
        m, d = np.load(out2 / "mels-ori" / (u + ".npy")), np.load(out2 / "durations_MFA" / (u + ".npy"))
        assert m.tobytes() == want[u][0].cpu().numpy().tobytes()
        assert d.shape == (p,) and d.sum() == t and np.array_equal(d[:-1], durs[u][:-1]) and np.issubdtype(d.dtype, np.integer)
        e, lf = np.load(out2 / "en-ori" / (u + ".npy")), np.load(out2 / "f0-ori" / (u + ".npy"))
        assert e.shape == lf.shape == (p,) and e.dtype == lf.dtype == np.float32
        e_want = F.segment_means(want[u][1].cpu().numpy().astype(np.float64), d)
        assert np.abs(e - e_want).max() <= (d.max() + 2) * U * np.abs(e_want).max()
        f = f0s[u][:t]
        lf_want = F.segment_means(np.where(f > 0, np.log(np.maximum(f, 1e-300)), 0.0), d, f)
        assert lf[0] == 0.0 and np.abs(lf - lf_want).max() <= (d.max() + 4) * U * np.abs(lf_want).max()
        mn, en, fn = (np.load(out2 / k / (u + ".npy")) for k in ("mels", "en", "f0"))
        assert mn.shape == (t, 80) and en.shape == fn.shape == (p, 1) and mn.dtype == en.dtype == fn.dtype == np.float32 and fn[0, 0] == 0.0
        assert np.allclose(en[:, 0], (e - fe[2]) / (fe[3] + 1e-8), rtol=1e-6, atol=1e-6)
        assert np.allclose(fn[lf != 0, 0], (lf[lf != 0] - fe[0]) / (fe[1] + 1e-8), rtol=1e-6, atol=1e-6) and (fn[lf == 0, 0] == 0).all()
    train_mels = np.concatenate([np.load(out2 / "mels" / (u + ".npy")) for u in ("ua", "uc")]).astype(np.float64)
    assert np.abs(train_mels.mean(0)).max() < 1e-5 and np.abs(train_mels.std(0) - 1.0).max() < 1e-5
    ori = np.concatenate([np.load(out2 / "mels-ori" / (u + ".npy")) for u in ("ua", "uc")]).astype(np.float64)
    assert np.allclose(mel_stats[0], ori.mean(0), atol=1e-9) and np.allclose(mel_stats[1], ori.std(0), atol=1e-7)
    lf_all = np.concatenate([np.load(out2 / "f0-ori" / (u + ".npy")) for u in ("ua", "uc")]).astype(np.float64)
    en_all = np.concatenate([np.load(out2 / "en-ori" / (u + ".npy")) for u in ("ua", "uc")]).astype(np.float64)
    assert np.allclose(fe, [lf_all[lf_all != 0].mean(), lf_all[lf_all != 0].std(), en_all.mean(), en_all.std()], rtol=1e-9)

    # durations and statistics without F0: en_stats.npy
    out3 = tmp_path / "o3"
    X.main(["--wav-dir", str(wavs), "--feature-root", str(out3), "--durations-dir", str(ddir), "--train-list", str(tmp_path / "train.txt"), "--verbose", "0"])
    assert sorted(p.name for p in out3.iterdir()) == ["durations_MFA", "en", "en-ori", "en_stats.npy", "mel_stats.npy", "mels", "mels-ori"]
    assert np.allclose(np.load(out3 / "en_stats.npy"), fe[2:], rtol=1e-12) and np.array_equal(np.load(out3 / "mel_stats.npy"), mel_stats)

    # a manifest over the written files is what the training driver reads
    utts = {}
    for u, t, p in zip(ids, T, P):
        inp = [dict(name="input%d" % (i + 1), feat=str(out2 / k / (u + ".npy")), shape=s)
               for i, (k, s) in enumerate((("mels", [t, 80]), ("durations_MFA", [p, 1]), ("f0", [p, 1]), ("en", [p, 1])))]
        utts[u] = dict(input=inp, output=[dict(name="target1", tokenid=" ".join(str(1 + (j % 40)) for j in range(p)), shape=[p, 41])])
    (tmp_path / "data.json").write_text(json.dumps({"utts": utts}))
    man = train.read_train_manifest(str(tmp_path / "data.json"))
    xs_, ys, _, ds, f0b, enb = train.load_batch(man)
    assert sorted(len(x) for x in xs_) == sorted(P) and [len(x) for x in xs_] == [len(d) for d in ds] == [len(f) for f in f0b] == [len(e) for e in enb]
    assert sorted(y.shape for y in ys) == sorted((t, 80) for t in T) and all(int(d.sum()) == y.shape[0] for d, y in zip(ds, ys))
    short = tmp_path / "short"
    short.mkdir()
    _write_wav(short / "tiny.wav", R.signal(1, 512))
    with pytest.raises(ValueError, match="utterance tiny has 512 samples"):
        X.main(["--wav-dir", str(short), "--feature-root", str(tmp_path / "o4"), "--verbose", "0"])
