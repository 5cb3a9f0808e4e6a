"""Float64 numpy statement of the F0 tracker (include/fcl_hip.h "F0 tracking"): no torch, no package code.  YIN (de Cheveigne &
Kawahara 2002) steps 1 - 5 on the frame grid of tests/features_ref.py: T = L // hop + 1 reflect-padded centred frames of N samples without a window,
d(tau) = sum_{j < N / 2} (x[j] - x[j + tau])^2 for tau <= tau_max + 1, the cumulative-mean normalisation d', the first dip below the threshold followed
downhill, a parabola through its three neighbours, F0 = fs / (tau + delta), and the removal of voiced runs shorter than min_voiced frames.

The inputs of tests/test_gpu_pitch.py are built here (GEOMETRIES, utterances), with the bounds the device results are held to, the frames on which
those bounds cannot decide the pick (fragile frames) and the mutants the bounds have to reject, so that tests/test_pitch_cpu.py can check all of that
without a GPU.

Bounds: derived, not measured.  U = 2^-24, gamma(n) = n U / (1 - n U) (Higham, Accuracy and Stability of Numerical Algorithms, Lemma 3.1), W = N / 2.
The device's inputs are the float32 samples themselves, so the only errors are its own roundings.
  d(tau).  The kernel sums the squared differences directly (csrc/pitch.hip): a difference is rounded once, its square enters an FMA exactly, and a
      term then passes through at most W + 2 additions (its segment's chain, then the segments in order).  All terms are non-negative, so
          |delta d(tau)| <= gamma(W + 4) d(tau) <= 2 gamma(W + 4) (e(0) + e(tau)) = beta (e(0) + e(tau)),
      since d <= 2 (e(0) + e(tau)).  The first form is the one used: the error is relative to d(tau) ITSELF, which is what keeps d' accurate inside a
      dip.  A correlation by two complex FFT passes (griffinlim_ref.fft_bound per pass, norm-wise) instead bounds |delta c(tau)| only by about
      1.5 sqrt(N) fft_bound(N) (e(0) + E), E the whole frame's energy: 5e-4 of the frame's energy at N = 1024, which is 10 - 100 % of d(tau) inside a
      dip and larger than the difference between the two lags next to a dip's minimum whenever the period exceeds ~100 samples; with that bound most
      voiced frames below 200 Hz would count as fragile.  That is why the direct sum was built, and no FFT term appears below.
  prefix sum S(tau) = sum_{j = 1 .. tau} d(j).  Blocks of 8 lags are summed in ascending order, the block totals in ascending order, and a block's
      offset is added to its running sums: a term passes through at most tau // 8 + 10 additions (a strictly sequential sum would pass through tau of them).  With the error of the terms,  |delta S| <= gamma(W + 4 + tau // 8 + 10) S.
  d'(tau) = fl(fl(d tau) / S): numerator gamma(W + 4) and one rounding, one rounding for the division, the denominator counted twice (Lemma 3.1):
          |delta d'(tau)| <= gamma(n(tau)) d'(tau),   n(tau) = (W + 4) + 2 + 2 (W + 4 + tau // 8 + 10).                            (cmnd_bound)
      Where S = 0 (digital silence) both sides give exactly 1, and d'(0) = 1.
  pick.  A frame is FRAGILE when a comparison the float64 pick actually made could come out differently within those bounds: some |d'(tau) - threshold|
      <= 2 b(tau), or some |d'(tau + 1) - d'(tau)| <= 2 max(b(tau), b(tau + 1)) (>= b(tau) + b(tau + 1), the error of the difference).  On every other
      frame the device must pick the same tau.
  F0 = fs / (tau + delta), delta = (a - c) / (2 D), D = a - 2 b + c, on values within ba, bb, bc of the float64 ones: with E = ba + 2 bb + bc and D > 2 E,
          |delta delta| <= ((ba + bc) + |a - c| E / D) / (2 (D - E))  +  8 U (|a| + 2 |b| + |c|) / D      (the last term: the fp32 evaluation),
      else 1 (both deltas lie in [-1/2, 1/2]); clamping is 1-Lipschitz.  |delta F0| / F0 <= |delta delta| / (tau + delta - |delta delta|) + 4 U.   (f0_bound)"""
import functools

import numpy as np

import features_ref as F

U = 2.0 ** -24
THRESHOLD, MIN_VOICED = 0.1, 3
# (fs, hop, N, f0_floor, f0_ceil)
GEOMETRIES = [(22050, 256, 1024, 71.0, 800.0), (22050, 300, 1024, 71.0, 800.0), (22050, 256, 512, 100.0, 800.0), (16000, 200, 512, 71.0, 800.0)]
GLIDES = [(90.0, 140.0), (120.0, 260.0), (220.0, 180.0), (300.0, 520.0), (75.0, 75.0), (700.0, 780.0)]
AMPS = (1.0, 0.6, 0.4, 0.3, 0.2, 0.1)


def gamma(n):
    return n * U / (1.0 - n * U)


# ---- the statement ---------------------------------------------------------------------------------------------------------------------------
def tau_range(fs, n, f0_floor, f0_ceil):
    """(tau_min, tau_max) = (floor(fs / f0_ceil), ceil(fs / f0_floor)); the contract needs 2 <= tau_min < tau_max <= n / 2 - 1"""
    return int(np.floor(fs / f0_ceil)), int(np.ceil(fs / f0_floor))


def frames_of(n_samples, hop):
    return int(n_samples) // int(hop) + 1


def frame_matrix(x, n, hop):
    """[T, n] float64: frame t holds the samples t * hop - n / 2 + j, reflected outside the utterance; no window"""
    return F.frame_matrix(x, n, hop)


def difference(fr, n_lag, wrap=False):
    """d [T, n_lag]: d(tau) = sum_{j < W} (x[j] - x[j + tau])^2, W = n / 2.  wrap (a mutant): W = n with the index j + tau taken modulo n"""
    n = fr.shape[1]
    if wrap:
        return np.stack([((fr - np.roll(fr, -tau, axis=1)) ** 2).sum(axis=1) for tau in range(n_lag)], axis=1)
    W = n // 2
    return np.stack([((fr[:, :W] - fr[:, tau : tau + W]) ** 2).sum(axis=1) for tau in range(n_lag)], axis=1)


def cmnd(d):
    """d' [T, n_lag]: d'(0) = 1, d'(tau) = d(tau) tau / sum_{j = 1 .. tau} d(j), 1 where that sum is 0"""
    out = np.ones_like(d)
    S = np.cumsum(d[:, 1:], axis=1)
    tau = np.arange(1, d.shape[1], dtype=np.float64)
    live = S > 0
    out[:, 1:][live] = (d[:, 1:] * tau)[live] / S[live]
    return out


def pick(dp, tau_min, tau_max, threshold=THRESHOLD, bound=None, first_dip=True):
    """one frame's d' [>= tau_max + 2] -> (tau, fragile): tau = 0 for an unvoiced frame.  The threshold is compared as the float32 the device holds.
    bound [like dp]: fragile = some comparison made here lies within twice the bound.  first_dip False (a mutant): the global minimum of d' over
    the range, as YIN's step 4 falls back to when no dip is below the threshold -- no frame is unvoiced then."""
    thr = float(np.float32(threshold))
    b = np.zeros_like(dp) if bound is None else bound
    fragile = False
    if not first_dip:
        return tau_min + int(np.argmin(dp[tau_min : tau_max + 1])), False
    tau = 0
    for t in range(tau_min, tau_max + 1):
        fragile |= abs(dp[t] - thr) <= 2 * b[t]
        if dp[t] < thr:
            tau = t
            break
    if tau == 0:
        return 0, bool(fragile)
    while tau < tau_max:
        fragile |= abs(dp[tau + 1] - dp[tau]) <= 2 * max(b[tau], b[tau + 1])
        if not dp[tau + 1] < dp[tau]:
            break
        tau += 1
    return tau, bool(fragile)


def parabola(a, b, c):
    """delta = (a - c) / (2 (a - 2 b + c)) clamped to [-1/2, 1/2]; 0 when the denominator is <= 0"""
    D = a - 2.0 * b + c
    return float(np.clip(0.5 * (a - c) / D, -0.5, 0.5)) if D > 0 else 0.0


def f0_of(dp, tau, fs, interpolate=True):
    if tau == 0:
        return 0.0
    return fs / (tau + (parabola(dp[tau - 1], dp[tau], dp[tau + 1]) if interpolate else 0.0))


def short_runs(f0, min_voiced=MIN_VOICED):
    """one utterance's track: voiced runs shorter than min_voiced frames become 0"""
    out = np.array(f0, copy=True)
    v = np.concatenate([[False], out != 0, [False]])
    starts, ends = np.flatnonzero(v[1:] & ~v[:-1]), np.flatnonzero(~v[1:] & v[:-1])
    for a, b in zip(starts, ends):
        if b - a < min_voiced:
            out[a:b] = 0
    return out


# ---- bounds ----------------------------------------------------------------------------------------------------------------------------------------
def cmnd_bound(dp, n):
    """|delta d'(tau)| per element (the docstring's derivation); 0 where d' is exactly 1 by rule"""
    W = n // 2
    tau = np.arange(dp.shape[-1])
    return gamma((W + 4) + 2 + 2 * (W + 4 + tau // 8 + 10)) * dp


def d_beta(n):
    """the energy-relative form: |delta d(tau)| <= beta (e(0) + e(tau)), beta = 2 gamma(W + 4)"""
    return 2.0 * gamma(n // 2 + 4)


def delta_bound(a, b, c, ba, bb, bc):
    """|delta_gpu - delta| for the device's fp32 parabola on values within ba, bb, bc of a, b, c"""
    D, E = a - 2.0 * b + c, ba + 2.0 * bb + bc
    if not D > 2.0 * E:
        return 1.0
    return min(1.0, ((ba + bc) + abs(a - c) * E / D) / (2.0 * (D - E)) + 8.0 * U * (abs(a) + 2.0 * abs(b) + abs(c)) / D)


def f0_bound(dp, bound, tau):
    """relative: |F0_gpu - F0| / F0 on a frame where both picked tau"""
    dd = delta_bound(dp[tau - 1], dp[tau], dp[tau + 1], bound[tau - 1], bound[tau], bound[tau + 1])
    return dd / (tau + parabola(dp[tau - 1], dp[tau], dp[tau + 1]) - dd) + 4.0 * U


def track(x, geo, threshold=THRESHOLD, wrap=False, raw=False, first_dip=True, interpolate=True):
    """one utterance -> dict(dp [T, tau_max + 2], bound, e0 [T], energy [T] (the whole frame's), tau [T], f0 [T] before the short-run removal, fragile [T], f0_bound [T]).
    The keywords are the mutants: wrap (W = N, circular), raw (d in place of d'), first_dip False (global minimum), interpolate False."""
    fs, hop, n, lo, hi = geo
    tau_min, tau_max = tau_range(fs, n, lo, hi)
    fr = frame_matrix(np.asarray(x, dtype=np.float64), n, hop)
    d = difference(fr, tau_max + 2, wrap)
    dp = d if raw else cmnd(d)
    bound = cmnd_bound(dp, n)
    T = len(fr)
    tau, fragile, f0, fb = np.zeros(T, dtype=np.int64), np.zeros(T, dtype=bool), np.zeros(T), np.zeros(T)
    for t in range(T):
        tau[t], fragile[t] = pick(dp[t], tau_min, tau_max, threshold, bound[t], first_dip)
        f0[t] = f0_of(dp[t], tau[t], float(fs), interpolate)
        if tau[t]:
            fb[t] = f0_bound(dp[t], bound[t], tau[t])
    return dict(dp=dp, bound=bound, e0=(fr[:, : n // 2] ** 2).sum(axis=1), energy=(fr ** 2).sum(axis=1), tau=tau, f0=f0, fragile=fragile, f0_bound=fb)


# ---- the inputs of tests/test_gpu_pitch.py --------------------------------------------------------------------------------------------------------
def glides_of(geo):
    """the glides whose both ends lie inside the geometry's F0 range"""
    return [g for g in GLIDES if geo[3] <= min(g) and max(g) <= geo[4]]


def harmonic(fs, f_inst, rng, noise_db=30.0):
    """six harmonics of the instantaneous fundamental f_inst [L] (Hz) with random phases, times 0.2, plus Gaussian noise noise_db below"""
    phase = 2.0 * np.pi * np.cumsum(f_inst) / fs
    s = sum(a * np.sin((k + 1) * phase + rng.uniform(0.0, 2.0 * np.pi)) for k, a in enumerate(AMPS)) * 0.2
    return s + rng.randn(len(s)) * np.sqrt(np.mean(s ** 2)) * 10.0 ** (-noise_db / 20.0)


def glide_parts(geo):
    """(harmonic, noise, zeros) sample counts of a glide utterance"""
    _, hop, n, _, _ = geo
    return 40 * hop + 7, 12 * hop, n + 2 * hop


def glide_f_inst(geo, g):
    Lh = glide_parts(geo)[0]
    return np.linspace(g[0], g[1], Lh)


def tone_hz(geo):
    """the constant fundamental of the three small utterances: a period of floor(fs / 220) + 1/2 samples, so that the first dip falls between two
    lags and the second on one"""
    return geo[0] / (np.floor(geo[0] / 220.0) + 0.5)


def burst_range(geo):
    """the samples of the fifth kind of utterance that carry the tone: silence before and after"""
    _, hop, n, _, _ = geo
    a = 3 * hop + n // 2  # frame 3 + n / (2 hop) starts here
    return a, a + n // 2 + int(np.ceil(geo[0] / tone_hz(geo))) + hop + hop // 2


@functools.lru_cache(maxsize=None)
def utterances(geo):
    """[(name, x float32)]: the glides inside the range, then 'shortest' (N / 2 + 1 samples), 'odd' (an odd frame count) and 'burst' (one isolated
    voiced stretch of 2 frames between silences)"""
    fs, hop, n, _, _ = geo
    gi = GEOMETRIES.index(geo)
    out = []
    for g in glides_of(geo):
        rng = np.random.RandomState(1000 * gi + GLIDES.index(g))
        Lh, Ln, Lz = glide_parts(geo)
        out.append(("glide %g-%g" % g, np.concatenate([harmonic(fs, glide_f_inst(geo, g), rng), rng.randn(Ln) * 0.05, np.zeros(Lz)])))
    f = tone_hz(geo)
    rng = np.random.RandomState(1000 * gi + 100)
    out.append(("shortest", harmonic(fs, np.full(n // 2 + 1, f), rng)))
    out.append(("odd", harmonic(fs, np.full(2 * n + 4 * hop + 3 + (hop if frames_of(2 * n + 4 * hop + 3, hop) % 2 == 0 else 0), f), rng)))
    a, b = burst_range(geo)
    x = np.zeros(b + n + 3 * hop)
    x[a:b] = harmonic(fs, np.full(b - a, f), rng)
    out.append(("burst", x))
    out = [(name, x.astype(np.float32)) for name, x in out]
    for _, x in out:
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(geo):
    """computed once per geometry and shared: [(name, x, track(x))] with read-only arrays"""
    out = []
    for name, x in utterances(geo):
        r = track(x, geo)
        for v in r.values():
            v.setflags(write=False)
        out.append((name, x, r))
    return out
