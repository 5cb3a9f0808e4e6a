"""Float64 numpy statement of the feature extraction (include/fcl_hip.h "Feature extraction"): no torch, no package code.  The forward
half of tests/griffinlim_ref.py: reflect-pad n_fft / 2, T = L // hop + 1 frames, periodic Hann zero-padded centred to n_fft, rfft, abs, the Slaney
area-normalised filterbank, log10(max(1e-10, .)); the frame energy is the 2-norm of the magnitudes.

The inputs of tests/test_gpu_features.py are built here (CASES, lengths, signals), with the bounds the device results are held to and the mutants
those bounds have to reject, so that tests/test_features_cpu.py can check all of that without a GPU."""
import numpy as np

import griffinlim_ref as R

U = R.U24
CASES = R.CASES + [R.SHORT_WINDOW_CASE]
FS, N_MELS, FMIN, FMAX = 22050, 80, 80.0, 7600.0
FLOOR = 1e-10


# ---- the statement ---------------------------------------------------------------------------------------------------------------------------
def frames_of(n_samples, hop):
    return int(n_samples) // int(hop) + 1


def frame_matrix(x, n_fft, hop, pad="reflect"):
    """[T, n_fft]: frame t holds the samples t * hop - n_fft / 2 + n of x, reflected (or zero) outside it; any L >= n_fft / 2 + 1"""
    x = np.asarray(x, dtype=np.float64)
    h = n_fft // 2
    assert len(x) >= h + 1
    xp = np.concatenate([x[1 : h + 1][::-1], x, x[-h - 1 : -1][::-1]]) if pad == "reflect" else np.concatenate([np.zeros(h), x, np.zeros(h)])
    return np.stack([xp[t * hop : t * hop + n_fft] for t in range(frames_of(len(x), hop))])


def spectrum(x, window, hop, pad="reflect"):
    """C [T, n_fft / 2 + 1] complex"""
    return np.fft.rfft(frame_matrix(x, len(window), hop, pad) * window, axis=1)


def features(x, window, hop, B, stats=None, pad="reflect"):
    """-> (S [T, F] magnitudes, E [T] energy, log-mel [T, n_mels]); stats [2, n_mels]: (v - mean) / (std + 1e-8) behind the log"""
    S = np.abs(spectrum(x, window, hop, pad))
    lm = np.log10(np.maximum(FLOOR, S @ np.asarray(B, dtype=np.float64).T))
    if stats is not None:
        lm = (lm - np.asarray(stats[0], dtype=np.float64)) / (np.asarray(stats[1], dtype=np.float64) + 1e-8)
    return S, np.linalg.norm(S, axis=1), lm


def segment_means(v, durations, mask=None):
    """one utterance: v [T], durations [P] summing to T -> [P] means over each phoneme's frames (only where mask != 0 when given); empty: 0"""
    v = np.asarray(v, dtype=np.float64)
    out, a = [], 0
    for d in durations:
        seg = v[a : a + int(d)]
        if mask is not None:
            seg = seg[np.asarray(mask[a : a + int(d)]) != 0]
        out.append(seg.mean() if len(seg) else 0.0)
        a += int(d)
    assert a == len(v)
    return np.asarray(out)


# ---- bounds: derived, not measured ------------------------------------------------------------------------------------------------------------
def magnitude_bound(S, n_fft):
    """per frame: ||S_gpu - S||_2 <= fft_bound ||C||_2 (|.| is 1-Lipschitz, and ||C||_2 = ||S||_2)"""
    return R.fft_bound(n_fft) * np.linalg.norm(S, axis=1)


def energy_bound(S, n_fft):
    """|dE| <= (fft_bound + 4 U) E: the norm is 1-Lipschitz in S; 4 U for the sum of squares and the root"""
    return (R.fft_bound(n_fft) + 4 * U) * np.linalg.norm(S, axis=1)


def logmel_bound(S, B, n_fft):
    """per element, M = S B^T:  dM = ||B_c||_2 fft_bound ||C_t||_2 + (nnz_c + 2) U M  (Cauchy-Schwarz on the magnitudes' error; the fp32 FMA chain
    over the channel's nnz_c bins and the rounding of its weights);  |d log10| <= dM / (M ln 10) + 4 U max(1, |log10 M|)  (log10f and the rounding
    of its result).  Where M <= 2e-10 -- at or next to the floor -- only the second term applies."""
    B = np.asarray(B, dtype=np.float64)
    M = S @ B.T
    nnz = (B != 0).sum(axis=1)
    dM = np.linalg.norm(B, axis=1)[None, :] * R.fft_bound(n_fft) * np.linalg.norm(S, axis=1)[:, None] + (nnz[None, :] + 2) * U * M
    Mf = np.maximum(FLOOR, M)
    tail = 4 * U * np.maximum(1.0, np.abs(np.log10(Mf)))
    return np.where(M <= 2 * FLOOR, tail, dM / (Mf * np.log(10.0)) + tail)


# ---- mutants: what a wrong rule would compute ----------------------------------------------------------------------------------------------------
def symmetric_hann(win_length, n_fft):
    out = np.zeros(n_fft)
    lp = (n_fft - win_length) // 2
    out[lp : lp + win_length] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win_length) / (win_length - 1))
    return out


def htk_filterbank(fs, n_fft, n_mels, fmin, fmax):
    """triangles between edges equally spaced on the HTK scale 2595 log10(1 + f / 700), area-normalised like the Slaney ones"""
    to_mel = lambda f: 2595.0 * np.log10(1.0 + np.asarray(f, dtype=np.float64) / 700.0)
    edges = 700.0 * (10.0 ** (np.linspace(to_mel(fmin), to_mel(fmax), n_mels + 2) / 2595.0) - 1.0)
    return _triangles(edges, fs, n_fft, True)


def unnormalised_filterbank(fs, n_fft, n_mels, fmin, fmax):
    """the Slaney triangles with peak 1 (no area normalisation)"""
    return _triangles(R.mel_centres(n_mels, fmin, fmax), fs, n_fft, False)


def _triangles(edges, fs, n_fft, area):
    freqs = np.linspace(0.0, fs / 2.0, n_fft // 2 + 1)
    B = np.zeros((len(edges) - 2, n_fft // 2 + 1))
    for i in range(len(edges) - 2):
        lo, c, hi = edges[i : i + 3]
        B[i] = np.maximum(0.0, np.minimum((freqs - lo) / (c - lo), (hi - freqs) / (hi - c))) * (2.0 / (hi - lo) if area else 1.0)
    return B


# ---- the inputs of tests/test_gpu_features.py ------------------------------------------------------------------------------------------------------
def lengths(case):
    """the shortest allowed length, two lengths hop does not divide, and one it does"""
    n_fft, hop, _ = case
    return [n_fft // 2 + 1, 40 * hop + 7, max(3 * hop - 1, n_fft // 2 + hop + 3), 2 * n_fft + 5 * hop]


def silent_range(case):
    """the samples of the fourth utterance that are set to zero: 2 - 3 wholly silent frames"""
    n_fft, hop, _ = case
    return n_fft // 2 + hop, n_fft // 2 + hop + n_fft + 2 * hop


def signals(case):
    """four utterances, rounded to float32"""
    out = [R.signal(17 * j, L).astype(np.float32) for j, L in enumerate(lengths(case))]
    a, b = silent_range(case)
    out[3][a:b] = 0.0
    return out


def filterbank(case):
    return R.mel_filterbank(FS, case[0], N_MELS, FMIN, FMAX)


def stats_case():
    """mel_stats like preprocessing's: [2, n_mels] (mean, std)"""
    return R.mel_case()[1]
