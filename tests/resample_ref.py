"""The resampling contract of include/fcl_hip.h "Resampling"  restated in float64 numpy, independent of the package: the ratio, the
Kaiser-windowed sinc (its Bessel function summed from the power series here), the coefficient table, the output length and the sum itself, with the
absolute sum the GPU tests' bound needs.  tests/test_resample_cpu.py checks this file against closed-form facts; tests/test_gpu_resample.py checks
csrc/resample.hip against it."""
import math

import numpy as np

ZEROS, ROLLOFF, BETA = 64, 0.9475937167399596, 14.769656459379492
U = 2.0 ** -24
PAIRS = [(48000, 22050), (16000, 22050), (44100, 22050), (22050, 16000)]  # the GPU cases: down with a table above LDS, up (s = 1), L = 1, down with L 320


def ratio(fs_in, fs_out):
    g = math.gcd(fs_in, fs_out)
    return fs_out // g, fs_in // g


def half_width(L, M):
    s = min(1.0, L / M)
    K = int(math.ceil(ZEROS / s))
    assert K == (ZEROS if M <= L else -((-ZEROS * M) // L))  # the float and the integer form agree
    return K


def bessel_i0(v):
    """I0 from its power series sum_k ((v / 2)^k / k!)^2: all terms positive, converged to the last bit well before k = 60 for v <= 15"""
    v = np.asarray(v, dtype=np.float64)
    term, total = np.ones_like(v), np.ones_like(v)
    for k in range(1, 80):
        term = term * (v / 2.0) / k
        total = total + term * term
    return total


def h(tau, s):
    tau = np.asarray(tau, dtype=np.float64)
    u = s * tau / ZEROS
    inside = np.abs(u) < 1.0
    win = bessel_i0(BETA * np.sqrt(np.where(inside, 1.0 - u * u, 0.0))) / bessel_i0(BETA)
    return np.where(inside, s * ROLLOFF * np.sinc(s * ROLLOFF * tau) * win, 0.0)


def table(L, M):
    """c [L][2 K + 1]: c[p][j + K] = h(j + p / L)"""
    K = half_width(L, M)
    j = np.arange(-K, K + 1, dtype=np.float64)
    return np.stack([h(j + p / L, min(1.0, L / M)) for p in range(L)])


def out_samples(n_in, L, M):
    return (n_in * L) // M


def resample(x, L, M, c=None):
    """x [n_in] -> (y [n_out], a [n_out]) in float64: y[t] = sum_j c[p][j] x[n - j], a[t] = sum_j |c[p][j] x[n - j]|, n = (t M) // L, p = (t M) mod L,
    samples outside [0, n_in) zero"""
    x = np.asarray(x, dtype=np.float64)
    K = half_width(L, M)
    c = table(L, M) if c is None else c
    n_out = out_samples(len(x), L, M)
    if n_out == 0:
        return np.zeros(0), np.zeros(0)
    t = np.arange(n_out, dtype=np.int64)
    n, p = (t * M) // L, (t * M) % L
    pad = int(n.max()) + 2 * K + 1
    xp = np.zeros(K + max(pad, len(x) + K) + 1)
    xp[K : K + len(x)] = x
    idx = (n[:, None] + K) - np.arange(-K, K + 1, dtype=np.int64)[None, :]  # x[n - j] in the padded array
    prod = c[p] * xp[idx]
    return prod.sum(axis=1), np.abs(prod).sum(axis=1)


def bound(a, K):
    """|y_float32 - y| <= (2 K + 3) 2^-24 sum_j |c x|: a (2 K + 1)-term float32 fma chain (gamma_{2K+1}) plus the rounding of each coefficient to
    float32 (one more u per product), to first order"""
    return (2 * K + 3) * U * a


def edge_skip(K, L, M):
    """outputs at either end whose filter reaches past the signal: K fs_out / fs_in + 2"""
    return int(K * L / M) + 2
