"""The evaluation contract of include/fcl_hip.h "Evaluation"  in float64 numpy: the DCT table with the folded de-normalisation, the
cepstra, the local distance, the DTW recurrence with its tie-break, the backtrack and the figures.  Every function takes a dtype, so that the same
statement can be run in float32 (the exact-arithmetic cases, the error model).  It also builds the inputs of test_evaluate_cpu.py and
test_gpu_evaluate.py; references are computed once per case and shared read-only."""
import functools
import math

import numpy as np

ORDER, ORDER_MAX, FRAMES_MAX = 13, 40, 4096
MCD_SCALE = 10.0 * math.sqrt(2.0) / math.log(10.0)
U = 2.0 ** -24

SIZES = [(1, 1), (1, 7), (7, 1), (2, 3), (63, 65), (64, 64), (65, 130), (5, 300), (300, 5), (257, 200), (300, 511)]
ORDERS = (13, 40)
KINDS = ("noise", "warp")


# ---- cepstra ------------------------------------------------------------------------------------------------------------------------------------
def dct_rows(N, D):
    """W [D][N]: W[k - 1][m] = sqrt(2 / N) cos(pi k (m + 1/2) / N), k = 1 .. D"""
    return np.array([[math.sqrt(2.0 / N) * math.cos(math.pi * k * (m + 0.5) / N) for m in range(N)] for k in range(1, D + 1)])


def table_bias(N, D, stats=None):
    """c = table x + bias: ln10 W on the log10 mels; stats ([2, N]: mean, std): x is normalised, x_raw = x (std + 1e-8) + mean"""
    raw = math.log(10.0) * dct_rows(N, D)
    if stats is None:
        return raw, np.zeros(D)
    stats = np.asarray(stats, dtype=np.float64)
    return raw * (stats[1] + 1e-8)[None, :], raw @ stats[0]


def cepstra(x, table, bias):
    """x [F][N] -> (c [F][D], sum_m |table[k][m] x[m]| [F][D]) in float64"""
    x, table = np.asarray(x, dtype=np.float64), np.asarray(table, dtype=np.float64)
    return x @ table.T + np.asarray(bias, dtype=np.float64)[None, :], np.abs(x) @ np.abs(table).T


def cepstra_bound(absum, bias, N):
    """(N + 2) 2^-24 sum_m |table[k][m] x[m]| + 2^-24 |bias_k|: N roundings of the fma chain and one of the final addition, on a float32-rounded
    table (the reference takes the rounded table, so its rounding does not count), and one spare"""
    return (N + 2) * U * absum + U * np.abs(np.asarray(bias, dtype=np.float64))[None, :]


# ---- DTW ----------------------------------------------------------------------------------------------------------------------------------------
def distances(a, b, dtype=np.float64):
    """d [Ta][Tb] = sqrt(sum_k (a_i[k] - b_j[k])^2), the sum in ascending k, every operation in dtype"""
    a, b = np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype)
    acc = np.zeros((a.shape[0], b.shape[0]), dtype=dtype)
    for k in range(a.shape[1]):
        df = a[:, k][:, None] - b[:, k][None, :]
        acc = acc + df * df
    return np.sqrt(acc)


def dp_loops(d):
    """the recurrence as a plain double loop -> (C, back-pointers: 0 diagonal, 1 (i - 1, j), 2 (i, j - 1))"""
    Ta, Tb = d.shape
    C = np.zeros_like(d)
    bp = np.zeros((Ta, Tb), dtype=np.uint8)
    inf = d.dtype.type(np.inf)
    for i in range(Ta):
        for j in range(Tb):
            if i == 0 and j == 0:
                C[0, 0] = d[0, 0]
                continue
            best, mv = (C[i - 1, j - 1], 0) if i > 0 and j > 0 else (inf, 0)
            if i > 0 and C[i - 1, j] < best:
                best, mv = C[i - 1, j], 1
            if j > 0 and C[i, j - 1] < best:
                best, mv = C[i, j - 1], 2
            C[i, j] = d[i, j] + best
            bp[i, j] = mv
    return C, bp


def dp(d):
    """the same, one anti-diagonal at a time"""
    Ta, Tb = d.shape
    C = np.full((Ta + 1, Tb + 1), np.inf, dtype=d.dtype)  # C[i + 1, j + 1]; row and column 0 are the predecessors outside the matrix
    bp = np.zeros((Ta, Tb), dtype=np.uint8)
    C[1, 1] = d[0, 0]
    for k in range(1, Ta + Tb - 1):
        i = np.arange(max(0, k - Tb + 1), min(k, Ta - 1) + 1)
        j = k - i
        best, mv = C[i, j].copy(), np.zeros(len(i), dtype=np.uint8)
        up, left = C[i, j + 1], C[i + 1, j]
        m = up < best
        best[m], mv[m] = up[m], 1
        m = left < best
        best[m], mv[m] = left[m], 2
        C[i + 1, j + 1] = d[i, j] + best
        bp[i, j] = mv
    return C[1:, 1:], bp


def backtrack(bp):
    """from (Ta - 1, Tb - 1) to (0, 0), in forward order: [n][2]"""
    i, j = bp.shape[0] - 1, bp.shape[1] - 1
    out = [(i, j)]
    while i or j:
        mv = bp[i, j]
        i, j = i - (mv != 2), j - (mv != 1)
        out.append((i, j))
    return np.array(out[::-1], dtype=np.int64)


def dtw(a, b, dtype=np.float64):
    """-> (cost C(Ta - 1, Tb - 1), path [n][2])"""
    C, bp = dp(distances(a, b, dtype))
    return C[-1, -1], backtrack(bp)


def is_warping_path(path, Ta, Tb):
    """starts at (0, 0), ends at (Ta - 1, Tb - 1), every step one of (1, 1), (1, 0), (0, 1)"""
    path = np.asarray(path, dtype=np.int64)
    if path.ndim != 2 or path.shape[1] != 2 or not max(Ta, Tb) <= len(path) <= Ta + Tb - 1:
        return False
    if tuple(path[0]) != (0, 0) or tuple(path[-1]) != (Ta - 1, Tb - 1):
        return False
    st = np.diff(path, axis=0)
    return bool(((st >= 0) & (st <= 1)).all() and (st.sum(axis=1) >= 1).all())


def path_cost(d, path):
    """the distances along a path summed as the recurrence sums them along it: c = d + c, in d's dtype"""
    c = d[path[0, 0], path[0, 1]]
    for i, j in path[1:]:
        c = d[i, j] + c
    return c


def gamma(Ta, Tb, D):
    """1.01 (Ta + Tb + D + 2) 2^-24: a path has at most Ta + Tb - 1 cells, so a cost is a chain of at most Ta + Tb - 2 float32 additions, and each
    distance carries D + 2 roundings of its sum and a half of its square root, first order, with 1 % for the higher orders"""
    return 1.01 * (Ta + Tb + D + 2) * U


def mcd_db(cost, n):
    return MCD_SCALE * float(cost) / n


# ---- pitch --------------------------------------------------------------------------------------------------------------------------------------
def cents(f0):
    f0 = np.asarray(f0, dtype=np.float64)
    return np.where(f0 > 0, 1200.0 * np.log2(np.maximum(f0, 1e-300)), 0.0)


def pitch_figures(path, pa, pb):
    """-> (n_vv, n_vuv, S) over the path's cells, in float64"""
    pa, pb = np.asarray(pa, dtype=np.float64)[path[:, 0]], np.asarray(pb, dtype=np.float64)[path[:, 1]]
    va, vb = pa > 0, pb > 0
    vv = va & vb
    return int(vv.sum()), int((va != vb).sum()), float(((pa - pb)[vv] ** 2).sum())


def f0_rmse(S, n_vv):
    return math.sqrt(S / n_vv) if n_vv else float("nan")


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------------
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def gaussian_pair(size, D, kind):
    """float32-rounded Gaussian cepstra: noise against noise, or b = a jittered, repeated-frame warp of a (a sorted random choice of a's frames,
    so that some repeat and some are skipped) plus noise of a tenth of its spread"""
    Ta, Tb = size
    rng = np.random.RandomState(1000 * Ta + 10 * Tb + D + (7 if kind == "warp" else 0))
    a = rng.randn(Ta, D).astype(np.float32)
    if kind == "noise":
        b = rng.randn(Tb, D).astype(np.float32)
    else:
        idx = np.sort(np.clip(np.rint(np.linspace(0, Ta - 1, Tb) + rng.uniform(-1.5, 1.5, Tb)), 0, Ta - 1).astype(np.int64))
        b = (a[idx] + 0.1 * rng.randn(Tb, D)).astype(np.float32)
    return _frozen(a, b)


@functools.lru_cache(maxsize=None)
def reference(size, D, kind):
    """dict(a, b, d64 [Ta][Tb], C64, path64) of a Gaussian pair, read-only"""
    a, b = gaussian_pair(size, D, kind)
    d = distances(a, b)
    C, bp = dp(d)
    path = backtrack(bp)
    _frozen(d, path)
    return dict(a=a, b=b, d=d, cost=float(C[-1, -1]), path=path)


# all-ties matrices: two constant sequences (d the same everywhere): the diagonal wins wherever it exists, so the path runs along the first
# row or column and then down the diagonal to the corner.  Written out by hand.
TIES = {
    (3, 5): [(0, 0), (0, 1), (0, 2), (1, 3), (2, 4)],
    (5, 3): [(0, 0), (1, 0), (2, 0), (3, 1), (4, 2)],
    (4, 4): [(0, 0), (1, 1), (2, 2), (3, 3)],
}


@functools.lru_cache(maxsize=None)
def exact_cases():
    """[(name, a [Ta][1], b [Tb][1])] float32 with integer values, |v| <= 64, lengths <= 40: every distance |a_i - b_j| <= 128 and every cumulative
    cost (at most 79 cells) is an integer below 2^24, exact in float32 in any order"""
    rng = np.random.RandomState(11)
    out = []
    for Ta, Tb in ((1, 1), (1, 9), (9, 1), (17, 23), (40, 40), (40, 13), (8, 40)):
        out.append(("int%dx%d" % (Ta, Tb), rng.randint(-64, 65, (Ta, 1)).astype(np.float32), rng.randint(-64, 65, (Tb, 1)).astype(np.float32)))
    for Ta, Tb in ((12, 12), (20, 31)):  # few distinct values: many ties inside the matrix
        out.append(("few%dx%d" % (Ta, Tb), rng.randint(0, 3, (Ta, 1)).astype(np.float32), rng.randint(0, 3, (Tb, 1)).astype(np.float32)))
    for (Ta, Tb) in TIES:
        out.append(("same%dx%d" % (Ta, Tb), np.full((Ta, 1), 3, np.float32), np.full((Tb, 1), 3, np.float32)))
        out.append(("apart%dx%d" % (Ta, Tb), np.full((Ta, 1), 2, np.float32), np.full((Tb, 1), 5, np.float32)))
    for _, a, b in out:
        _frozen(a, b)
    return out


def pitch_inputs(kind, n, rng):
    """cents [n] float32: random in [6500, 11600] with random unvoiced runs / all unvoiced / all voiced"""
    p = rng.uniform(6500.0, 11600.0, n).astype(np.float32)
    if kind == "unvoiced":
        p[:] = 0
    elif kind == "runs":
        k = 0
        while k < n:
            run = int(rng.randint(1, 9))
            if rng.rand() < 0.4:
                p[k : k + run] = 0
            k += run
    return p


def harmonic_with_gap(fs, n, hz, rng, gap=(0.4, 0.7)):
    """a tone of six decaying harmonics at hz[0] -> hz[1] with a silent stretch inside, |x| < 1"""
    f = np.linspace(hz[0], hz[1], n)
    ph = 2.0 * np.pi * np.cumsum(f) / fs
    x = sum(0.6 ** k * np.sin((k + 1) * ph + rng.uniform(0, 2 * np.pi)) for k in range(6)) * 0.2
    x = x + rng.randn(n) * 1e-3
    x[int(gap[0] * n) : int(gap[1] * n)] = rng.randn(int(gap[1] * n) - int(gap[0] * n)) * 1e-4
    return x
