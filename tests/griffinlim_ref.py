"""Float64 numpy statement of the Griffin-Lim vocoder (include/fcl_hip.h "Griffin-Lim vocoder"): no torch, no package code.

Everything the GPU tests compare against is built here, and so are the exact inputs they use (CASES, utt_lens, signal, magnitudes, phase0), so
that tests/test_griffinlim_cpu.py can check the conditions those inputs have to meet without a GPU."""
import numpy as np

FLT_MIN = float(np.finfo(np.float32).tiny)
U24 = 2.0 ** -24


# ---- mel filterbank (Slaney scale, area normalisation) ---------------------------------------------------------------------------------
def hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3.0, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-300) / min_log_hz) / logstep, f / f_sp)


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3.0, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_centres(n_mels, fmin, fmax):
    """the n_mels + 2 band edges in Hz: equally spaced on the Slaney mel scale"""
    return mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), n_mels + 2))


def mel_filterbank(fs, n_fft, n_mels, fmin, fmax):
    """B [n_mels, n_fft / 2 + 1]: triangle i rises from edge i to edge i + 1 and falls to edge i + 2, scaled by 2 / (edge i + 2 - edge i)."""
    edges = mel_centres(n_mels, fmin, fmax)
    freqs = np.linspace(0.0, fs / 2.0, n_fft // 2 + 1)
    B = np.zeros((n_mels, n_fft // 2 + 1))
    for i in range(n_mels):
        lo, c, hi = edges[i], edges[i + 1], edges[i + 2]
        B[i] = np.maximum(0.0, np.minimum((freqs - lo) / (c - lo), (hi - freqs) / (hi - c))) * (2.0 / (hi - lo))
    return B


def mel_to_linear(mel, stats, pinv_t):
    """mel [frames, n_mels] (normalised log10 mel), stats [2, n_mels] or None, pinv_t = pinv(B)^T [n_mels, F] -> S [frames, F]"""
    lm = np.asarray(mel, dtype=np.float64)
    if stats is not None:
        lm = lm * (np.asarray(stats[1], dtype=np.float64) + 1e-8) + np.asarray(stats[0], dtype=np.float64)
    return np.maximum(1e-10, (10.0 ** lm) @ np.asarray(pinv_t, dtype=np.float64))


# ---- window, STFT, ISTFT ------------------------------------------------------------------------------------------------------------------
def hann_window(win_length, n_fft):
    """periodic Hann of win_length, zero-padded centred to n_fft"""
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win_length) / win_length)
    out = np.zeros(n_fft)
    lp = (n_fft - win_length) // 2
    out[lp : lp + win_length] = w
    return out


def frames_of(x, n_fft, hop):
    """explicit framing: reflect-pad n_fft / 2 on both sides, frame t starts at t * hop -> [T, n_fft], T = len(x) / hop + 1"""
    x = np.asarray(x, dtype=np.float64)
    h = n_fft // 2
    assert len(x) % hop == 0 and len(x) > h
    xp = np.concatenate([x[1 : h + 1][::-1], x, x[-h - 1 : -1][::-1]])
    T = len(x) // hop + 1
    return np.stack([xp[t * hop : t * hop + n_fft] for t in range(T)])


def stft(x, window, hop):
    n_fft = len(window)
    return np.fft.rfft(frames_of(x, n_fft, hop) * window, axis=1)


def window_sumsquare(window, hop, T):
    n_fft = len(window)
    wss = np.zeros(n_fft + hop * (T - 1))
    for t in range(T):
        wss[t * hop : t * hop + n_fft] += window ** 2
    return wss


def synth_frames(C, window):
    """inverse real FFT (imaginary parts of the DC and Nyquist bins ignored, as numpy.fft.irfft) times the window"""
    return np.fft.irfft(C, n=len(window), axis=1) * window


def overlap_add(fr, window, hop):
    T, n_fft = fr.shape
    buf = np.zeros(n_fft + hop * (T - 1))
    for t in range(T):
        buf[t * hop : t * hop + n_fft] += fr[t]
    wss = window_sumsquare(window, hop, T)
    ok = wss > FLT_MIN
    buf[ok] /= wss[ok]
    return buf[n_fft // 2 : len(buf) - n_fft // 2]


def istft(C, window, hop):
    return overlap_add(synth_frames(C, window), window, hop)


# ---- initial phase: counter-based uniforms --------------------------------------------------------------------------------------------------
def _hash_u32(x):
    x = np.asarray(x, dtype=np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def phase_uniforms(utt_seed, T, F):
    """u [T, F] float32 in [0, 1): h = hash(hash(seed ^ hash(t + 0x9E3779B9)) ^ (k * 0x85EBCA6B)), u = (h >> 8) * 2^-24 (all uint32, wrapping)"""
    with np.errstate(over="ignore"):
        t = np.arange(T, dtype=np.uint32) + np.uint32(0x9E3779B9)
        a = _hash_u32(np.uint32(int(utt_seed) & 0xFFFFFFFF) ^ _hash_u32(t))
        k = np.arange(F, dtype=np.uint32) * np.uint32(0x85EBCA6B)
        h = _hash_u32(a[:, None] ^ k[None, :])
    return ((h >> np.uint32(8)).astype(np.float32) * np.float32(U24)).astype(np.float32)


# ---- the iteration ----------------------------------------------------------------------------------------------------------------------------
def _r32(a):
    if np.iscomplexobj(a):
        return a.astype(np.complex64).astype(np.complex128)
    return a.astype(np.float32).astype(np.float64)


def griffin_lim(S, phase0, window, hop, n_iter, momentum, round32=False, trace=None):
    """One utterance: S [T, F] magnitudes, phase0 [T, F] complex unit phases -> waveform [hop * (T - 1)].  round32: every stored intermediate
    (frames, y, C, P) is rounded to float32 -- the model of the device's storage.  trace: optional dict receiving the last P, A and C."""
    r = _r32 if round32 else (lambda a: a)
    S = np.asarray(S, dtype=np.float64)
    P = r(np.asarray(phase0, dtype=np.complex128))
    Cp = np.zeros_like(P)
    alpha = momentum / (1.0 + momentum)
    for _ in range(n_iter):
        y = r(overlap_add(r(synth_frames(S * P, window)), window, hop))
        C = r(stft(y, window, hop))
        A = C - alpha * Cp
        P = r(A / (np.abs(A) + 1e-16))
        Cp = C
        if trace is not None:
            trace.update(P=P, A=A, C=C)
    return r(overlap_add(r(synth_frames(S * P, window)), window, hop))


def spectral_convergence(y, S, window, hop):
    return float(np.linalg.norm(np.abs(stft(y, window, hop)) - S) / np.linalg.norm(S))


def fft_bound(n_fft):
    """Higham's bound on the relative 2-norm error of a radix-2 FFT in fp32 with twiddles good to one ulp, plus one stage each for the window and
    the real-FFT split: 7 (log2(n_fft) + 2) 2^-24"""
    return 7.0 * (np.log2(n_fft) + 2.0) * U24


# ---- the inputs of tests/test_gpu_griffinlim.py ------------------------------------------------------------------------------------------------
# (n_fft, hop, win_length): every n_fft x hop n_fft / 4, n_fft / 2 and one hop that does not divide n_fft; one window shorter than n_fft
CASES = [(512, 128, 512), (512, 256, 512), (512, 100, 512), (1024, 256, 1024), (1024, 512, 1024), (1024, 300, 1024), (2048, 512, 2048),
         (2048, 1024, 2048), (2048, 300, 2048)]
SHORT_WINDOW_CASE = (1024, 512, 400)  # win_length < hop: between the windows of neighbouring frames the window-sum-square is exactly zero
ITER_CASE = (1024, 256, 1024)


def min_frames(n_fft, hop):
    """the shortest utterance whose reflection is a single one: T >= n_fft / (2 hop) + 2 (n_fft / (2 hop) rounded up for a hop that does not divide)"""
    return -(-n_fft // (2 * hop)) + 2


def utt_lens(n_fft, hop):
    """shortest allowed T, T + 1 and one of about 40 frames"""
    t = min_frames(n_fft, hop)
    return [t, 41, t + 1]


def signal(seed, n):
    """a few partials with slow amplitude modulation over a noise floor 20 dB below them per bin: no bin of the spectrum is tiny against the largest, so
    a phase comparison that skips |A| < 1e-3 max|A| skips next to nothing (test_griffinlim_cpu.py checks the share)"""
    rng = np.random.RandomState(seed)
    i = np.arange(n)
    x = sum(a * np.sin(2 * np.pi * f * i + p) for a, f, p in zip((0.12, 0.08, 0.05), (0.011, 0.057, 0.173), rng.uniform(0, 6.28, 3)))
    return x * (0.6 + 0.4 * np.sin(2 * np.pi * i / 977.0)) + 0.2 * rng.randn(n)


def case_signals(case, seed=0):
    n_fft, hop, _ = case
    return [signal(seed + 17 * j, hop * (T - 1)) for j, T in enumerate(utt_lens(n_fft, hop))]


def case_window(case):
    return hann_window(case[2], case[0])


def case_spectra(case, seed=0):
    """per utterance (S [T, F], P [T, F]): magnitudes of a real signal's STFT and independent random unit phases"""
    w = case_window(case)
    out = []
    for j, x in enumerate(case_signals(case, seed)):
        S = np.abs(stft(x, w, case[1]))
        rng = np.random.RandomState(1000 + seed + j)
        out.append((S, np.exp(2j * np.pi * rng.uniform(size=S.shape))))
    return out


def mel_case(seed=0, frames=37, n_mels=80):
    """normalised log-mel rows like a model's output, mel_stats like preprocess.py's, and one row that drives linear bins negative (a single hot mel
    channel: the pseudo-inverse's side lobes are negative)"""
    rng = np.random.RandomState(seed)
    mel = rng.randn(frames, n_mels) * 0.8
    stats = np.stack([-2.0 + 0.5 * rng.randn(n_mels), 0.6 + 0.2 * rng.rand(n_mels)])
    hot = np.full(n_mels, -3.0)
    hot[n_mels // 2] = 3.0
    mel[5] = hot
    return mel, stats
