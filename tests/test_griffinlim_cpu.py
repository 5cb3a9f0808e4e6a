"""CPU checks of the Griffin-Lim vocoder: the float64 reference against numpy's FFT, the filterbank's properties, the drivers' flags,
the refusals by name, samples_of of the three generators, and the conditions the GPU tests' own inputs (tests/griffinlim_ref.py) have to meet."""
import ctypes as C

import numpy as np
import pytest

import griffinlim_ref as R

ALL_CASES = R.CASES + [R.SHORT_WINDOW_CASE]


@pytest.fixture(scope="module")
def GL():
    from fcl_taco2_amd import griffinlim

    return griffinlim


def test_reference_stft_equals_rfft_of_explicit_frames():
    n_fft, hop = 512, 100
    x = R.signal(3, hop * 9)
    w = R.hann_window(n_fft, n_fft)
    h = n_fft // 2
    frames = []
    for t in range(10):
        idx = np.arange(t * hop - h, t * hop - h + n_fft)
        idx = np.where(idx < 0, -idx, idx)
        idx = np.where(idx >= len(x), 2 * (len(x) - 1) - idx, idx)  # a single reflection at either end
        frames.append(x[idx])
    frames = np.stack(frames)
    C_ = R.stft(x, w, hop)
    assert C_.shape == (10, h + 1) and np.abs(C_ - np.fft.rfft(frames * w, axis=1)).max() < 1e-12
    assert np.array_equal(R.frames_of(x, n_fft, hop), frames)


@pytest.mark.parametrize("case", ALL_CASES, ids=str)
def test_reference_round_trip(case):
    """istft(stft(x)) = x to 1e-12 for every geometry the GPU tests use (where the window-sum-square is not tiny: everywhere for the Hann cases)"""
    n_fft, hop, wl = case
    w = R.case_window(case)
    for x in R.case_signals(case):
        T = len(x) // hop + 1
        y = R.istft(R.stft(x, w, hop), w, hop)
        wss = R.window_sumsquare(w, hop, T)[n_fft // 2 : -(n_fft // 2)]
        ok = wss > 1e-3
        assert y.shape == x.shape == (hop * (T - 1),) and np.abs(y - x)[ok].max() < 1e-12
        if wl == n_fft:
            assert ok.all() and wss.min() > 0.1  # the Hann cases: the trimmed window-sum-square stays above 0.1
        else:
            assert (wss <= R.FLT_MIN).sum() > 0  # the short window really reaches the undivided branch


def test_utterance_lists_hold_the_shortest_allowed_lengths():
    for n_fft, hop, _ in ALL_CASES:
        lens = R.utt_lens(n_fft, hop)
        t = R.min_frames(n_fft, hop)
        assert 2 * hop * (t - 2) >= n_fft > 2 * hop * (t - 3) and lens == [t, 41, t + 1]
    # with a hop that does not divide n_fft the shortest utterance has a frame that reflects at BOTH ends
    n_fft, hop = 2048, 300
    t = R.min_frames(n_fft, hop)
    assert any(f * hop - n_fft // 2 < 0 and f * hop + n_fft // 2 > hop * (t - 1) for f in range(t))


def test_filterbank_properties(GL):
    for fs, n_fft, n_mels, fmin, fmax in [(22050, 1024, 80, 80.0, 7600.0), (16000, 512, 40, 0.0, 8000.0)]:
        B = R.mel_filterbank(fs, n_fft, n_mels, fmin, fmax)
        assert np.allclose(B, GL.mel_filterbank(fs, n_fft, n_mels, fmin, fmax), rtol=1e-12, atol=1e-15)  # the package builds the same matrix
        edges = R.mel_centres(n_mels, fmin, fmax)
        freqs = np.linspace(0, fs / 2.0, n_fft // 2 + 1)
        assert B.shape == (n_mels, n_fft // 2 + 1) and (B >= 0).all() and np.all(np.diff(edges) > 0)
        assert np.allclose(np.diff(R.hz_to_mel(edges)), np.diff(R.hz_to_mel(edges))[0])  # equally spaced on the mel scale
        for i in range(n_mels):
            lo, c, hi = edges[i : i + 3]
            inside = (freqs > lo) & (freqs < hi)
            assert np.all(B[i][~inside] == 0)
            up, down = inside & (freqs <= c), inside & (freqs >= c)
            # triangular: linear on both flanks, the (continuous) peak 2 / (hi - lo) at the centre
            assert np.allclose(B[i][up], (freqs[up] - lo) / (c - lo) * 2.0 / (hi - lo)) and np.allclose(B[i][down], (hi - freqs[down]) / (hi - c) * 2.0 / (hi - lo))
            assert B[i].max() <= 2.0 / (hi - lo) * (1 + 1e-12)
        peaks = [freqs[np.argmax(B[i])] for i in range(n_mels) if B[i].max() > 0]
        assert np.all(np.diff(peaks) >= 0)


def test_pinv_is_the_identity_on_the_row_space():
    B = R.mel_filterbank(22050, 1024, 80, 80.0, 7600.0)
    Pi = np.linalg.pinv(B)  # [F, n_mels]
    assert np.linalg.matrix_rank(B) == 80
    # a spectrum in the row space of B (S = c B) comes back from its mel (m = S B^T) exactly: m pinv(B)^T = S
    c = np.random.RandomState(0).rand(5, 80)
    S = c @ B
    assert np.abs((S @ B.T) @ Pi.T - S).max() < 1e-9 * np.abs(S).max()
    assert np.abs(B @ Pi - np.eye(80)).max() < 1e-9


def test_phase_uniforms_twin_matches_the_reference_statement(GL):
    for seed, T, F in [(0, 7, 513), (2 ** 32 - 1, 3, 257), (12345, 41, 1025)]:
        u, v = R.phase_uniforms(seed, T, F), GL.phase_uniforms(seed, T, F)
        assert u.dtype == np.float32 and u.tobytes() == v.tobytes() and 0 <= u.min() and u.max() < 1
    u = R.phase_uniforms(7, 64, 513)
    assert abs(u.mean() - 0.5) < 0.01 and not np.array_equal(u, R.phase_uniforms(8, 64, 513)) and not np.array_equal(u[0], u[1])


def test_window_and_twiddle_tables(GL):
    for n_fft, _, wl in ALL_CASES:
        assert np.array_equal(GL.hann_window(wl, n_fft), R.hann_window(wl, n_fft))
        tw = GL.twiddles(n_fft).astype(np.float64)
        ref = np.exp(-2j * np.pi * np.arange(n_fft) / n_fft)
        assert tw.shape == (n_fft, 2) and np.abs(tw[:, 0] + 1j * tw[:, 1] - ref).max() <= 2.0 ** -24  # good to one ulp (half an ulp of 1)
        assert tuple(tw[n_fft // 2]) == (-1.0, 0.0) and tuple(tw[n_fft // 4]) == (0.0, -1.0)
    assert np.array_equal(GL.window_sumsquare(R.hann_window(400, 1024), 512, 5), R.window_sumsquare(R.hann_window(400, 1024), 512, 5))


def test_parsers_and_flag_exclusivity(tmp_path):
    from fcl_taco2_amd import tts as TTS, vocoder_decode as V

    base_v = ["--feats-scp", "x.scp", "--outdir", "o"]
    base_t = ["--model", "m", "--model-conf", "c", "--json", "j", "--outdir", "o"]
    for parse, base, ck in ((V.parse_args, base_v, "--checkpoint"), (TTS.parse_args, base_t, "--vocoder-checkpoint")):
        a = parse(base + ["--griffin-lim"])
        assert a.griffin_lim and (a.fs, a.n_fft, a.hop, a.win_length, a.fmin, a.fmax, a.gl_iters, a.gl_momentum) == (22050, 1024, 256, None, 80.0, 7600.0, 64, 0.99)
        assert a.mel_stats is None and a.mel_basis is None
        a = parse(base + [ck, "g.pkl"])
        assert not a.griffin_lim
        a = parse(base + ["--griffin-lim", "--n-fft", "2048", "--hop", "300", "--win-length", "1200", "--gl-iters", "32", "--gl-momentum", "0", "--fs", "24000",
                          "--fmin", "0", "--fmax", "12000", "--mel-stats", "s.npy", "--mel-basis", "b.npy"])
        assert (a.n_fft, a.hop, a.win_length, a.gl_iters, a.gl_momentum, a.fs, a.fmax, a.mel_stats, a.mel_basis) == (2048, 300, 1200, 32, 0.0, 24000, 12000.0, "s.npy", "b.npy")
        for bad in (base, base + ["--griffin-lim", ck, "g.pkl"], base + ["--griffin-lim", "--n-fft", "768"], base + ["--griffin-lim", "--hop", "600"],
                    base + ["--griffin-lim", "--win-length", "2048"], base + ["--griffin-lim", "--gl-momentum", "1.5"]):
            with pytest.raises(SystemExit) as e:  # neither, both, or an unsupported geometry: an argparse error
                parse(bad)
            assert e.value.code == 2, bad


def test_refusals_by_name(GL):
    for kw, name in ((dict(n_fft=768), "n_fft"), (dict(n_fft=4096), "n_fft"), (dict(hop=0), "hop"), (dict(hop=513), "hop"), (dict(win_length=1025), "win_length"),
                     (dict(n_mels=300), "n_mels")):
        with pytest.raises(NotImplementedError, match=name):
            GL.GriffinLimPlan("cpu", **kw)  # refused before the device is looked at
    for kw, name in ((dict(fmax=12000.0), "fmax"), (dict(momentum=-0.1), "momentum"), (dict(n_iter=-1), "n_iter"), (dict(mel_stats=np.zeros((2, 79))), "mel_stats"),
                     (dict(mel_basis=np.zeros((80, 512))), "mel_basis")):
        with pytest.raises(ValueError, match=name):
            GL.GriffinLimPlan("cpu", **kw)
    from fcl_taco2_amd import _lib

    with pytest.raises(_lib.FclError, match="GPU"):
        GL.GriffinLimPlan("cpu")
    # an utterance below n_fft / (2 hop) + 2 frames is refused by id
    assert GL.min_frames(1024, 256) == 4 and GL.min_frames(2048, 300) == 6 and GL.min_frames(512, 256) == 3
    GL.check_lens([4, 9], 1024, 256, ["a", "b"])
    with pytest.raises(ValueError, match="utterance b has 3 frames"):
        GL.check_lens([4, 3], 1024, 256, ["a", "b"])
    with pytest.raises(ValueError, match="utterance #0 has 5 frames"):
        GL.check_lens([5, 40], 2048, 300)


def test_c_entries_validate_without_a_gpu():
    from fcl_taco2_amd import _lib

    lib = _lib.load()
    a = _lib.GriffinLim()
    entries = (lib.fcl_gl_phase_init, lib.fcl_gl_synth_fwd, lib.fcl_gl_ola_fwd, lib.fcl_gl_analysis_fwd)
    for fn in entries:
        assert fn(None, None) == -1
        a.n_fft, a.hop, a.frames, a.n_utt = 768, 256, 10, 1
        assert fn(C.byref(a), None) == -2 and b"n_fft must be 512, 1024 or 2048" in lib.fcl_last_error()
        a.n_fft, a.hop = 1024, 513
        assert fn(C.byref(a), None) == -2 and b"hop" in lib.fcl_last_error()
        a.hop, a.n_utt = 256, 11
        assert fn(C.byref(a), None) == -2 and b"n_utt" in lib.fcl_last_error()
        a.n_utt = 2
        assert fn(C.byref(a), None) == -1 and b"null" in lib.fcl_last_error()
    a.frame_utt = a.utt_off = a.y = a.window = a.twiddle = a.p = 256
    a.momentum = 0.99
    assert lib.fcl_gl_analysis_fwd(C.byref(a), None) == -1 and b"needs c_prev" in lib.fcl_last_error()
    a.momentum, a.p = 0.0, 260
    assert lib.fcl_gl_analysis_fwd(C.byref(a), None) == -3 and b"8-byte" in lib.fcl_last_error()
    assert lib.fcl_gl_mel2lin_fwd(None, None, None, None, 4, 80, 513, None) == -1
    assert lib.fcl_gl_mel2lin_fwd(256, None, 256, 256, 4, 300, 513, None) == -2 and b"n_mels" in lib.fcl_last_error()


def test_samples_of_for_all_three_generators(GL):
    from fcl_taco2_amd import hifigan, vocoder

    class P(object):
        hop = 256

    for cls in (vocoder.ParallelWaveGANGenerator, hifigan.HiFiGANGenerator):
        g = cls.__new__(cls)
        g.plan = P()
        assert [g.samples_of(n) for n in (1, 7, 40)] == [256, 7 * 256, 40 * 256]
    g = GL.GriffinLim.__new__(GL.GriffinLim)
    g.plan = P()
    assert [g.samples_of(n) for n in (4, 7, 40)] == [3 * 256, 6 * 256, 39 * 256] and GL.GriffinLimPlan.eager_only is True


def test_iteration_inputs_leave_out_at_most_one_percent_of_the_bins():
    """the phase comparison of the one- and two-iteration GPU test judges P where |A| >= 1e-3 max|A|: on its own inputs that leaves out <= 1 %"""
    case = R.ITER_CASE
    w = R.case_window(case)
    for n_iter in (1, 2):
        for S, P0 in R.case_spectra(case):
            tr = {}
            R.griffin_lim(S, P0, w, case[1], n_iter, 0.99, trace=tr)
            a = np.abs(tr["A"])
            assert (a < 1e-3 * a.max()).mean() <= 0.01


def test_mel_case_reaches_the_floor():
    mel, stats = R.mel_case()
    B = R.mel_filterbank(22050, 1024, 80, 80.0, 7600.0)
    pt = np.linalg.pinv(B).T.astype(np.float32).astype(np.float64)
    raw = (10.0 ** (mel.astype(np.float32).astype(np.float64) * (stats[1] + 1e-8) + stats[0])) @ pt
    assert (raw[5] < 0).sum() > 10 and (R.mel_to_linear(mel, stats, pt)[5] == 1e-10).sum() > 10
