"""CPU checks of the feature extraction: the conditions the GPU tests' own inputs (tests/features_ref.py) have to meet, for the
reference alone -- lengths, silent frames, the size of the bounds, the mutants those bounds reject -- and the host side of the package: the banded
filter tables, frames_of, the last-duration adjustment, the statistics and normalisation, the driver's argument errors and wav refusals, and the
C entries' validation, all without a GPU."""
import ctypes as C
import wave

import numpy as np
import pytest

import features_ref as F
import griffinlim_ref as R


@pytest.fixture(scope="module")
def FX():
    from fcl_taco2_amd import features

    return features


def _w(case):
    return R.hann_window(case[2], case[0])


@pytest.mark.parametrize("case", F.CASES, ids=str)
def test_inputs_meet_their_conditions(case):
    """every L >= n_fft / 2 + 1 with the shortest one present, lengths hop divides and does not; the fourth utterance has >= 2 frames with E == 0 and
    log-mel == -10, every other frame E > 0; the per-element log-mel bound stays <= 5e-3"""
    n_fft, hop, _ = case
    Ls = F.lengths(case)
    assert min(Ls) == Ls[0] == n_fft // 2 + 1 and Ls[1] % hop != 0 and Ls[2] % hop != 0 and all(L // hop + 1 <= 41 for L in Ls)
    assert Ls[3] % hop == 0 or n_fft % hop != 0  # hop divides the fourth length wherever it divides n_fft
    B, w = F.filterbank(case), _w(case)
    worst = 0.0
    for j, x in enumerate(F.signals(case)):
        assert x.dtype == np.float32 and len(x) == Ls[j]
        S, E, lm = F.features(x, w, hop, B)
        assert S.shape == (Ls[j] // hop + 1, n_fft // 2 + 1) and lm.shape == (S.shape[0], F.N_MELS)
        silent = E == 0
        assert silent.sum() >= 2 if j == 3 else not silent.any()
        assert (lm[silent] == -10.0).all() and (lm[~silent] > -10.0).all()
        bound = F.logmel_bound(S, B, n_fft)
        assert np.isfinite(bound).all() and (bound > 0).all()
        worst = max(worst, float(bound.max()))
    assert worst <= 5e-3


@pytest.mark.parametrize("case", F.CASES, ids=str)
def test_each_mutant_misses_ten_times_the_bound_on_every_utterance(case):
    """symmetric Hann, zero padding (first and last frame), the HTK scale and a filterbank without area normalisation, computed in numpy on the same
    inputs: each exceeds 10 x the log-mel bound on at least one element of every utterance; the window and padding mutants also 10 x the energy bound"""
    n_fft, hop, wl = case
    B, w = F.filterbank(case), _w(case)
    mutants = {
        "symmetric Hann": dict(window=F.symmetric_hann(wl, n_fft)),
        "zero padding": dict(pad="zero"),
        "HTK scale": dict(B=F.htk_filterbank(F.FS, n_fft, F.N_MELS, F.FMIN, F.FMAX)),
        "no area normalisation": dict(B=F.unnormalised_filterbank(F.FS, n_fft, F.N_MELS, F.FMIN, F.FMAX)),
    }
    for name, kw in mutants.items():
        margins = []
        for x in F.signals(case):
            S, E, lm = F.features(x, w, hop, B)
            S2, E2, lm2 = F.features(x, kw.get("window", w), hop, kw.get("B", B), pad=kw.get("pad", "reflect"))
            rows = [0, -1] if name == "zero padding" else slice(None)
            m_mel = float((np.abs(lm2 - lm) / F.logmel_bound(S, B, n_fft))[rows].max())
            margins.append(m_mel)
            assert m_mel > 10.0, (name, m_mel)
            if name in ("symmetric Hann", "zero padding"):
                live = E > 0
                m_en = float((np.abs(E2 - E)[live] / F.energy_bound(S, n_fft)[live]).max())
                assert m_en > 10.0, (name, m_en)
        print("%r %s: smallest margin over the log-mel bound %.3g" % (case, name, min(margins)))


def test_banded_tables_reproduce_the_dense_filterbank_exactly(FX):
    for fs, n_fft, n_mels, fmin, fmax in [(22050, 512, 80, 80.0, 7600.0), (22050, 1024, 80, 80.0, 7600.0), (22050, 2048, 80, 80.0, 7600.0), (16000, 512, 40, 0.0, 8000.0)]:
        B = R.mel_filterbank(fs, n_fft, n_mels, fmin, fmax)
        lo, off, w = FX.banded_filterbank(B)
        assert lo.dtype == off.dtype == np.int32 and len(lo) == n_mels and len(off) == n_mels + 1 and off[-1] == len(w) == (B != 0).sum()
        assert (lo + np.diff(off) <= n_fft // 2 + 1).all() and (w != 0).all()
        assert np.array_equal(FX.dense_filterbank(lo, off, w, n_fft // 2 + 1), B)
        w32 = w.astype(np.float32)  # what is uploaded
        assert np.array_equal(FX.dense_filterbank(lo, off, w32, n_fft // 2 + 1), B.astype(np.float32))
    gap = np.zeros((2, 9))
    gap[0, 1:4], gap[1, 2], gap[1, 5] = 1.0, 1.0, 1.0
    with pytest.raises(ValueError, match="row 1 is not a contiguous band"):
        FX.banded_filterbank(gap)
    with pytest.raises(ValueError, match="row 1 is not a contiguous band"):
        FX.FeaturePlan("cpu", n_fft=512, hop=128, mel_basis=np.pad(gap, ((0, 0), (0, 248))))
    lo, off, w = FX.banded_filterbank(np.array([[0.0, 0.0, 0.0], [0.0, 2.0, 3.0]]))  # an all-zero row is an empty run
    assert list(lo) == [0, 1] and list(off) == [0, 0, 2] and list(w) == [2.0, 3.0]


def test_frames_lengths_and_refusals(FX):
    from fcl_taco2_amd import _lib

    assert [FX.frames_of(n, 256) for n in (513, 767, 768, 10247)] == [3, 3, 4, 41] == [F.frames_of(n, 256) for n in (513, 767, 768, 10247)]
    assert FX.min_samples(1024) == 513
    FX.check_lens([513, 9000], 1024, ["a", "b"])
    with pytest.raises(ValueError, match="utterance b has 512 samples"):
        FX.check_lens([513, 512], 1024, ["a", "b"])
    with pytest.raises(ValueError, match="utterance #0 has 1024 samples"):
        FX.check_lens([1024], 2048)
    for kw, name in ((dict(n_fft=768), "n_fft"), (dict(hop=0), "hop"), (dict(hop=513), "hop"), (dict(win_length=1025), "win_length"), (dict(n_mels=300), "n_mels")):
        with pytest.raises(NotImplementedError, match=name):
            FX.FeaturePlan("cpu", **kw)
    for kw, name in ((dict(fmax=12000.0), "fmax"), (dict(mel_stats=np.zeros((2, 79))), "mel_stats"), (dict(mel_basis=np.zeros((80, 512))), "mel_basis")):
        with pytest.raises(ValueError, match=name):
            FX.FeaturePlan("cpu", **kw)
    with pytest.raises(_lib.FclError, match="GPU"):
        FX.FeaturePlan("cpu")  # no CPU fallback
    assert FX.DEFAULTS == dict(fs=22050, n_fft=1024, hop=256, win_length=None, n_mels=80, fmin=80.0, fmax=7600.0)


def test_last_duration_adjustment(FX):
    out = FX.adjust_durations([[3, 4, 5], [7], [2, 0, 9]], [14, 5, 8], ["a", "b", "c"])
    assert [list(d) for d in out] == [[3, 4, 7], [5], [2, 0, 6]] and all(d.dtype == np.int64 for d in out)
    with pytest.raises(ValueError, match="utterance b has 9 frames .* would be -1"):
        FX.adjust_durations([[1, 2], [6, 4, 3]], [3, 9], ["a", "b"])
    with pytest.raises(ValueError, match="utterance #0"):
        FX.adjust_durations([[]], [3])
    with pytest.raises(ValueError, match="utterance #0"):
        FX.adjust_durations([[4, -1, 2]], [5])


def test_statistics_and_normalisation_against_numpy():
    from fcl_taco2_amd import extract_features as X

    rng = np.random.RandomState(5)
    mels = [rng.randn(n, 7) * 2.0 - 3.0 for n in (11, 4, 23)]
    m = X.Moments()
    for a in mels:
        m.add(a)
    mean, std = m.result("mel")
    allm = np.concatenate(mels)
    assert np.allclose(mean, allm.mean(0), rtol=0, atol=1e-12) and np.allclose(std, allm.std(0), rtol=0, atol=1e-10)  # population standard deviation
    f0 = [np.array([0.0, 5.1, 5.3, 0.0]), np.array([4.9, 0.0])]
    m = X.Moments()
    for a in f0:
        m.add(a[a != 0.0])
    fm, fs = m.result("F0")
    voiced = np.array([5.1, 5.3, 4.9])
    assert abs(fm - voiced.mean()) < 1e-12 and abs(fs - voiced.std()) < 1e-10
    got = X.normalise(f0[0].reshape(-1, 1), fm, fs, nonzero_only=True)
    assert got.dtype == np.float32 and got.shape == (4, 1) and got[0, 0] == 0 and got[3, 0] == 0
    assert np.allclose(got[1:3, 0], (f0[0][1:3] - voiced.mean()) / (voiced.std() + 1e-8), rtol=1e-6)
    assert np.allclose(X.normalise(mels[1], mean, std), (mels[1] - allm.mean(0)) / (allm.std(0) + 1e-8), rtol=1e-6, atol=1e-6)
    with pytest.raises(ValueError, match="no voiced F0 entries"):
        X.Moments().result("voiced F0")
    lf = X.log_f0([0.0, 100.0, 220.0])
    assert lf.dtype == np.float32 and lf[0] == 0 and np.allclose(lf[1:], np.log([100.0, 220.0]))
    assert list(X.fit_track([1.0, 2.0, 3.0], 2)) == [1.0, 2.0] and list(X.fit_track([1.0], 3)) == [1.0, 0.0, 0.0]


def test_reference_segment_means():
    v = np.arange(10.0)
    assert np.allclose(F.segment_means(v, [3, 0, 7]), [1.0, 0.0, 6.0])
    mask = np.array([0, 1, 1, 0, 0, 0, 0, 0, 0, 1.0])
    assert np.allclose(F.segment_means(v, [3, 4, 3], mask), [1.5, 0.0, 9.0])


def _write_wav(path, pcm, rate=22050, width=2, channels=1):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(channels)
        f.setsampwidth(width)
        f.setframerate(rate)
        f.writeframes(np.asarray(pcm).tobytes())


def test_driver_argument_errors_and_wav_refusals(tmp_path):
    from fcl_taco2_amd import extract_features as X

    wavs, durs = tmp_path / "wavs", tmp_path / "durs"
    wavs.mkdir()
    durs.mkdir()
    (tmp_path / "train.txt").write_text("a\n")
    base = ["--wav-dir", str(wavs), "--feature-root", str(tmp_path / "out")]
    a = X.parse_args(base)
    assert (a.fs, a.n_fft, a.hop, a.win_length, a.n_mels, a.fmin, a.fmax, a.batch_frames) == (22050, 1024, 256, None, 80, 80.0, 7600.0, 51200)
    assert a.durations_dir is None and a.f0_dir is None and a.train_list is None
    a = X.parse_args(base + ["--durations-dir", str(durs), "--f0-dir", str(durs), "--train-list", str(tmp_path / "train.txt"), "--n-fft", "2048", "--hop", "300"])
    assert (a.n_fft, a.hop, a.durations_dir) == (2048, 300, str(durs))
    for bad in (["--feature-root", "o"], base + ["--wav-scp", "x.scp"], ["--wav-dir", str(wavs)], base + ["--f0-dir", str(durs)], base + ["--n-fft", "768"],
                base + ["--hop", "600"], base + ["--n-mels", "300"], base + ["--fmax", "12000"], base + ["--batch-frames", "0"],
                base + ["--durations-dir", str(tmp_path / "nowhere")], base + ["--train-list", str(tmp_path / "missing.txt")],
                base + ["--mel-stats", "s.npy"], base + ["--gl-iters", "3"], ["--wav-scp", str(tmp_path / "missing.scp"), "--feature-root", "o"]):
        with pytest.raises(SystemExit) as e:
            X.parse_args(bad)
        assert e.value.code == 2, bad
    pcm = (np.sin(np.arange(2000) * 0.05) * 8000).astype("<i2")
    _write_wav(wavs / "ok.wav", pcm)
    x = X.read_wav(str(wavs / "ok.wav"), 22050)
    assert x.dtype == np.float32 and np.array_equal(x, pcm.astype(np.float32) / 32768.0)
    _write_wav(wavs / "wide.wav", pcm.astype("<i4"), width=4)
    _write_wav(wavs / "stereo.wav", np.stack([pcm, pcm], axis=1), channels=2)
    _write_wav(wavs / "slow.wav", pcm, rate=16000)
    for name, what in (("wide", "4-byte samples"), ("stereo", "2 channels"), ("slow", "sampling rate 16000")):
        for fn in (X.read_wav, X.wav_samples):
            with pytest.raises(ValueError, match=r"%s\.wav: %s" % (name, what)):
                fn(str(wavs / (name + ".wav")), 22050)
    assert X.wav_samples(str(wavs / "ok.wav"), 22050) == 2000
    assert [u for u, _ in X.read_wav_list(wav_dir=str(wavs))] == ["ok", "slow", "stereo", "wide"]
    (tmp_path / "w.scp").write_text("u2 %s\nu1 %s\n" % (wavs / "ok.wav", wavs / "slow.wav"))
    assert X.read_wav_list(wav_scp=str(tmp_path / "w.scp")) == [("u1", str(wavs / "slow.wav")), ("u2", str(wavs / "ok.wav"))]


def test_c_entries_validate_without_a_gpu():
    from fcl_taco2_amd import _lib

    lib = _lib.load()
    assert lib.fcl_version() == _lib.ABI_VERSION  # new entries and a new struct only: no mirrored layout changed, the revision stays
    fn = lib.fcl_fx_logmel_fwd
    assert fn(None, None) == -1
    a = _lib.Features()
    a.n_fft, a.hop, a.frames, a.n_utt, a.n_mels, a.nnz, a.samples = 768, 256, 10, 1, 80, 100, 5000
    assert fn(C.byref(a), None) == -2 and b"n_fft must be 512, 1024 or 2048" in lib.fcl_last_error()
    a.n_fft, a.hop = 1024, 513
    assert fn(C.byref(a), None) == -2 and b"hop" in lib.fcl_last_error()
    a.hop, a.n_mels = 256, 257
    assert fn(C.byref(a), None) == -2 and b"n_mels" in lib.fcl_last_error()
    a.n_mels, a.nnz = 80, 0
    assert fn(C.byref(a), None) == -2 and b"nnz" in lib.fcl_last_error()
    a.nnz, a.n_utt = 100, 11
    assert fn(C.byref(a), None) == -2 and b"n_utt" in lib.fcl_last_error()
    a.n_utt, a.frames = 2, 2 ** 31 // 513 + 1
    assert fn(C.byref(a), None) == -2 and b"2^31" in lib.fcl_last_error()
    a.frames, a.samples = 10, 2 ** 31
    assert fn(C.byref(a), None) == -2 and b"samples" in lib.fcl_last_error()
    a.samples = 5000
    assert fn(C.byref(a), None) == -1 and b"null x" in lib.fcl_last_error()
    a.x = a.smp_off = a.frame_utt = a.utt_off = 256
    assert fn(C.byref(a), None) == -1 and b"null window" in lib.fcl_last_error()
    a.window = a.twiddle = a.fb_lo = a.fb_off = a.fb_w = 256
    assert fn(C.byref(a), None) == -1 and b"null mel / energy" in lib.fcl_last_error()
    a.mel = a.energy = 256
    a.window = 260
    assert fn(C.byref(a), None) == -3 and b"8-byte" in lib.fcl_last_error()
    sm = lib.fcl_fx_segment_mean_fwd
    assert sm(None, None, None, None, None, None, None, 4, 1, 10, 0, None) == -1 and b"null" in lib.fcl_last_error()
    assert sm(256, None, 256, 256, 256, 256, 256, 4, 1, 10, 1, None) == -1 and b"needs mask" in lib.fcl_last_error()
    assert sm(256, None, 256, 256, 256, 256, 256, 1, 2, 10, 0, None) == -2 and b"n_ph >= n_utt" in lib.fcl_last_error()
    assert sm(256, None, 256, 256, 256, 256, 256, 4, 2, 1, 0, None) == -2
    assert sm(256, None, 256, 256, 256, 256, 256, 2 ** 31, 2, 10, 0, None) == -2


def test_features_struct_layout_matches_the_header(tmp_path):
    import os
    import subprocess

    from conftest import ROOT
    from fcl_taco2_amd import _lib

    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fcl_hip.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(fcl_fx_t), '
                   'offsetof(fcl_fx_t, x), offsetof(fcl_fx_t, mag_out)); return 0; }\n')
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")], check=True)
    out = tuple(int(v) for v in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split())
    assert out == (C.sizeof(_lib.Features), _lib.Features.x.offset, _lib.Features.mag_out.offset)
