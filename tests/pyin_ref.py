"""Numpy statement of the probabilistic YIN tracker (include/fcl_hip.h "Probabilistic YIN"): no torch, no package code.  pYIN (Mauch &
Dixon 2014) on the d' of tests/pitch_ref.py: a Beta(2, 18) distribution over 100 thresholds turns one frame's d' row into several period candidates
with a probability each, binned on a log-frequency grid; a Viterbi pass over (voicing, bin) picks the track.

Every function takes the number format as an argument: np.float64 is the statement, np.float32 restates both launches of csrc/pyin.hip in their exact
operation order (every product, sum and quotient rounded on its own), so that the device's results can be compared bit for bit.  The only operation
numpy and the device do not share is the logarithm: lv and lu are held to K_LOG ulp of the float64 logarithm instead.

K_LOG: tools/probe/pyin_log_ulp.hip measured the device's logf against float64 over [1e-30, 1] (2^22 points, log-spaced, plus every power of two and
its neighbours), in units of the ulp of the result's binade: worst error LOG_WORST_ULP = 2.1409 ulp (at 0.00375).  By DESIGN 6m's rule, twice the
worst error rounded up to a power of two: K_LOG = 8.

Viterbi bounds (DESIGN 6i's form): a path's score is a sum of 3 T - 2 float32 additions (tri, la and the observation per frame), so with
gamma = 1.01 (3 T + 2) 2^-24 and A the sum of the |terms| along a path, the float32 score of ANY path is within gamma A of its float64 sum.  Hence the
device's score is within gamma A of the float64 sum along its own path, and the float64 optimum V64 exceeds that sum by at most 2.1 gamma A (the
device's path beat the float64-optimal one in float32; both float32 scores are within gamma A' of their float64 sums, A' <= 1.05 A)."""
import functools

import numpy as np

import pitch_ref as P

PA, FLOOR = 0.01, 1e-30
N_THR = 100
BINS_PER_SEMITONE, MAX_RATE = 5, 35.92
LOG_WORST_ULP, K_LOG = 2.1409, 8
INNER = (3, 57)  # the swell signal's inner frames 3 .. 56
TAIL = 63        # its tail frames: index >= 63


# ---- tables ------------------------------------------------------------------------------------------------------------------------------------
def beta_cdf(x):
    """the Beta(2, 18) cdf"""
    x = np.asarray(x, dtype=np.float64)
    return 1.0 - (1.0 - x) ** 18 * (1.0 + 18.0 * x)


def tables(fs, hop, f0_floor, f0_ceil, bins_per_semitone=BINS_PER_SEMITONE, max_rate=MAX_RATE, dtype=np.float64):
    """dict(thr [100], cw [101], nb, f_bin [nb], edge [nb - 1], W, tri [2 W + 1], la [2, 2]): built in float64, then converted to dtype.  thr is what
    the device compares with: the float32 value of i / 100 in either format."""
    i = np.arange(1, N_THR + 1, dtype=np.float64)
    w = beta_cdf(i / N_THR) - beta_cdf((i - 1.0) / N_THR)
    steps = 12.0 * bins_per_semitone
    nb = int(np.floor(steps * np.log2(f0_ceil / f0_floor))) + 1
    W = int(np.round(max_rate * steps * hop / fs))
    k = np.arange(2 * W + 1, dtype=np.float64)
    tb = dict(thr=(i / N_THR).astype(np.float32).astype(np.float64), cw=np.concatenate([[0.0], np.cumsum(w)]),
              f_bin=f0_floor * 2.0 ** (np.arange(nb) / steps), edge=fs / (f0_floor * 2.0 ** ((np.arange(nb - 1) + 0.5) / steps)),
              tri=np.log((W + 1.0 - np.abs(k - W)) / (W + 1.0) ** 2), la=np.log(np.array([[0.99, 0.01], [0.01, 0.99]])))
    tb = {name: v.astype(dtype) for name, v in tb.items()}
    tb.update(nb=nb, W=W, fs=float(fs))
    return tb


def geo_tables(geo, dtype=np.float64):
    fs, hop, _, lo, hi = geo
    return tables(fs, hop, lo, hi, dtype=dtype)


# ---- launch 1: one frame's d' -> observations --------------------------------------------------------------------------------------------------
def candidates(dp, tau_min, tau_max, tb, dtype=np.float64):
    """one frame's d' -> [(m, mass)] in ascending lag: the walk of the contract"""
    thr, cw = tb["thr"], tb["cw"]
    dp = np.asarray(dp, dtype=dtype)
    out, rec, rec_i, t, lo_i = [], dtype(np.inf), N_THR, tau_min, N_THR
    while t <= tau_max:
        if dp[t] < rec:
            m = t
            while m < tau_max and dp[m + 1] < dp[m]:
                m += 1
            lo_i = int(np.count_nonzero(thr <= dp[m]))
            out.append((m, dtype(cw[rec_i] - cw[lo_i])))
            rec, rec_i, t = dp[m], lo_i, m + 1
        else:
            t += 1
    if out:
        m, mass = out[-1]
        out[-1] = (m, dtype(mass + dtype(dtype(PA) * cw[lo_i])))
    return out


def period(dp, m, dtype=np.float64):
    """p = m + delta in the contract's operation order"""
    a, b, c = dtype(dp[m - 1]), dtype(dp[m]), dtype(dp[m + 1])
    D = dtype(dtype(a - dtype(b + b)) + c)
    delta = dtype(0.0)
    if D > 0:
        delta = dtype(dtype(dtype(0.5) * dtype(a - c)) / D)
        delta = min(max(delta, dtype(-0.5)), dtype(0.5))
    return dtype(dtype(m) + delta)


def observe_frame(dp, tau_min, tau_max, tb, dtype=np.float64):
    """-> (ov [nb], bf0 [nb], pv, bins): the probability mass per pitch bin, each bin's F0 (that of its heaviest candidate, the first among equals; 0
    where no candidate with mass fell), their sum over ascending bins and the candidates' bins"""
    nb = tb["nb"]
    ov, best, bf0, bins = np.zeros(nb, dtype=dtype), np.zeros(nb, dtype=dtype), np.zeros(nb, dtype=dtype), []
    for m, mass in candidates(dp, tau_min, tau_max, tb, dtype):
        p = period(dp, m, dtype)
        b = int(np.count_nonzero(tb["edge"] >= p))
        bins.append(b)
        ov[b] = dtype(ov[b] + mass)
        if mass > best[b]:
            best[b], bf0[b] = mass, dtype(dtype(tb["fs"]) / p)
    pv = dtype(0.0)
    for b in range(nb):
        pv = dtype(pv + ov[b])
    return ov, bf0, pv, bins


def log_obs(ov, pv, nb, dtype=np.float64):
    """(lv [nb], lu) of one frame: ln max(ov, FLOOR) and ln max((1 - pv) / nb, FLOOR)"""
    u = dtype(dtype(dtype(1.0) - pv) / dtype(nb))
    return np.log(np.maximum(ov, dtype(FLOOR))), np.log(max(u, dtype(FLOOR)))


def observe(dp, tau_min, tau_max, tb, dtype=np.float64):
    """d' [T, >= tau_max + 2] -> dict(ov [T, nb], bf0 [T, nb], pv [T], lv [T, nb], lu [T], bins [T lists])"""
    T, nb = len(dp), tb["nb"]
    out = dict(ov=np.zeros((T, nb), dtype), bf0=np.zeros((T, nb), dtype), pv=np.zeros(T, dtype), lv=np.zeros((T, nb), dtype), lu=np.zeros(T, dtype), bins=[])
    for t in range(T):
        ov, bf0, pv, bins = observe_frame(dp[t], tau_min, tau_max, tb, dtype)
        out["ov"][t], out["bf0"][t], out["pv"][t] = ov, bf0, pv
        out["lv"][t], out["lu"][t] = log_obs(ov, pv, nb, dtype)
        out["bins"].append(bins)
    return out


# ---- launch 2: Viterbi over (voicing, bin) ------------------------------------------------------------------------------------------------------
def viterbi(lv, lu, tb, dtype=np.float64):
    """lv [T, nb], lu [T] -> (state [T] int, score, V [2 nb] of the last frame): state = v * nb + b, v = 0 voiced.  Vectorised over the bins."""
    lv, lu = np.asarray(lv, dtype=dtype), np.asarray(lu, dtype=dtype)
    T, nb = lv.shape
    W, tri, la = tb["W"], tb["tri"].astype(dtype), tb["la"].astype(dtype)
    K = 2 * W + 1
    V = np.stack([lv[0], np.full(nb, lu[0], dtype=dtype)])
    bp = np.zeros((T, 2, nb), dtype=np.int64)
    pad = np.full((2, nb + 2 * W), -np.inf, dtype=dtype)
    for t in range(1, T):
        pad[:, W : W + nb] = V
        M, Mk = np.full((2, nb), -np.inf, dtype=dtype), np.full((2, nb), W, dtype=np.int64)
        for k in range(K):
            c = pad[:, k : k + nb] + tri[k]
            up = c > M
            M[up], Mk[up] = c[up], k
        for v2 in range(2):
            c0, c1 = M[0] + la[0, v2], M[1] + la[1, v2]
            one = c1 > c0
            V[v2] = np.where(one, c1, c0) + (lv[t] if v2 == 0 else lu[t])
            bp[t, v2] = np.where(one, K + Mk[1], Mk[0])
    return backtrack(V.reshape(-1), bp.reshape(T, 2 * nb), nb, W)


def backtrack(Vlast, bp, nb, W):
    """the largest V wins, the lowest index among equals; code = v1 (2 W + 1) + k leads to (v1, b + k - W)"""
    T, K = len(bp), 2 * W + 1
    state = np.zeros(T, dtype=np.int64)
    s = int(np.argmax(Vlast))
    for t in range(T - 1, -1, -1):
        state[t] = s
        code = int(bp[t, s])
        s = (code // K) * nb + min(max(s % nb + code % K - W, 0), nb - 1)
    return state, Vlast[state[-1]], Vlast


def viterbi_loops(lv, lu, tb, dtype=np.float64):
    """the same recurrence as a plain triple loop over frame, state and predecessor"""
    lv, lu = np.asarray(lv, dtype=dtype), np.asarray(lu, dtype=dtype)
    T, nb = lv.shape
    W, tri, la = tb["W"], tb["tri"].astype(dtype), tb["la"].astype(dtype)
    K = 2 * W + 1
    V = np.concatenate([lv[0], np.full(nb, lu[0], dtype=dtype)])
    bp = np.zeros((T, 2 * nb), dtype=np.int64)
    for t in range(1, T):
        Vn = np.zeros_like(V)
        for s in range(2 * nb):
            v2, b = divmod(s, nb)
            M, Mk = [dtype(-np.inf)] * 2, [W, W]
            for v1 in range(2):
                for k in range(K):
                    if 0 <= b + k - W < nb:
                        c = dtype(V[v1 * nb + b + k - W] + tri[k])
                        if c > M[v1]:
                            M[v1], Mk[v1] = c, k
            c0, c1 = dtype(M[0] + la[0, v2]), dtype(M[1] + la[1, v2])
            Vn[s] = dtype((c1 if c1 > c0 else c0) + (lv[t, b] if v2 == 0 else lu[t]))
            bp[t, s] = K + Mk[1] if c1 > c0 else Mk[0]
        V = Vn
    return backtrack(V, bp, nb, W)


def path_terms(state, lv, lu, tb):
    """the float64 terms added along a path, in order: the start's observation, then tri, la and the observation of every later frame"""
    lv, lu = np.asarray(lv, dtype=np.float64), np.asarray(lu, dtype=np.float64)
    nb, W, tri, la = lv.shape[1], tb["W"], tb["tri"].astype(np.float64), tb["la"].astype(np.float64)
    terms = []
    for t, s in enumerate(state):
        v, b = divmod(int(s), nb)
        if t:
            v1, b1 = divmod(int(state[t - 1]), nb)
            assert abs(b - b1) <= W
            terms += [tri[b1 - b + W], la[v1, v]]
        terms.append(lv[t, b] if v == 0 else lu[t])
    return np.asarray(terms)


def gamma_path(T):
    return 1.01 * (3 * T + 2) * 2.0 ** -24


def decode_f0(state, bf0, tb):
    """a voiced state's F0: that of its bin's heaviest candidate, the bin's centre where none fell; 0 for an unvoiced state"""
    nb = tb["nb"]
    out = np.zeros(len(state), dtype=bf0.dtype)
    for t, s in enumerate(state):
        if s < nb:
            out[t] = bf0[t, s] if bf0[t, s] > 0 else tb["f_bin"][s]
    return out


# ---- the whole tracker ----------------------------------------------------------------------------------------------------------------------------
def track_dp(dp, geo, dtype=np.float64, min_voiced=P.MIN_VOICED):
    """d' [T, tau_max + 2] of one utterance -> dict(f0 [T] after the short-run removal, raw, state, score, obs)"""
    fs, _, n, lo, hi = geo
    tau_min, tau_max = P.tau_range(fs, n, lo, hi)
    tb = geo_tables(geo, dtype)
    obs = observe(np.asarray(dp, dtype=dtype), tau_min, tau_max, tb, dtype)
    state, score, _ = viterbi(obs["lv"], obs["lu"], tb, dtype)
    raw = decode_f0(state, obs["bf0"], tb)
    return dict(f0=P.short_runs(raw, min_voiced), raw=raw, state=state, score=score, obs=obs)


def track(x, geo):
    """one utterance's samples -> the float64 statement's result (track_dp on pitch_ref's d')"""
    return track_dp(P.track(x, geo)["dp"], geo)


def yin_track(x, geo):
    """plain YIN with the short-run removal: what the feature is compared with"""
    return P.short_runs(P.track(x, geo)["f0"])


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------------
SWELL_HZ, SWELL_FRAMES = 150.0, 60


@functools.lru_cache(maxsize=None)
def swell(geo, seed):
    """a steady 150 Hz tone whose 2nd and 4th harmonics swell over the frames [20, 30), 12 frames at -3 dB SNR from frame 40, then 8 frames of faint
    noise: float32, read-only"""
    fs, hop = geo[0], geo[1]
    rng = np.random.RandomState(seed)
    L = SWELL_FRAMES * hop
    phase = 2.0 * np.pi * SWELL_HZ * np.arange(L) / fs
    amps = np.tile(np.asarray(P.AMPS, dtype=np.float64)[:, None], (1, L))
    win = np.hanning(10 * hop)
    amps[1, 20 * hop : 30 * hop] += 6.0 * win
    amps[3, 20 * hop : 30 * hop] += 2.0 * win
    s = 0.2 * sum(amps[k] * np.sin((k + 1) * phase + rng.uniform(0.0, 2.0 * np.pi)) for k in range(len(P.AMPS)))
    r = np.sqrt(np.mean((0.2 * sum(a * np.sin((k + 1) * phase) for k, a in enumerate(P.AMPS))) ** 2))
    g = np.full(L, 10.0 ** (-30.0 / 20.0))
    g[40 * hop : 52 * hop] = 10.0 ** (-3.0 / 20.0)
    s = s + rng.randn(L) * r * g
    x = np.concatenate([s, rng.randn(8 * hop) * 0.01]).astype(np.float32)
    x.setflags(write=False)
    return x


def wrong_inner(f0):
    """how many of the inner frames are unvoiced or more than 3 % off 150 Hz"""
    v = np.asarray(f0, dtype=np.float64)[INNER[0] : INNER[1]]
    return int(np.count_nonzero((v == 0) | (np.abs(v / SWELL_HZ - 1.0) > 0.03)))


def voiced_tail(f0):
    return int(np.count_nonzero(np.asarray(f0)[TAIL:] != 0))


@functools.lru_cache(maxsize=None)
def swell_reference(geo, seed):
    """computed once and shared: dict(x, dp, f64 = track_dp in float64, yin = YIN + short-run removal)"""
    x = swell(geo, seed)
    r = P.track(x, geo)
    return dict(x=x, dp=r["dp"], f64=track_dp(r["dp"], geo), yin=P.short_runs(r["f0"]))


# ---- the Viterbi launch's own cases ---------------------------------------------------------------------------------------------------------------
VITERBI_CASES = [(1, 1, 1), (1, 1, 5), (2, 1, 2), (13, 3, 1), (13, 20, 7), (64, 5, 63), (64, 5, 64), (64, 5, 65), (127, 25, 300), (128, 25, 9), (129, 25, 9),
                 (210, 25, 1), (210, 25, 2), (210, 29, 517), (257, 25, 40), (512, 63, 130)]


def band_tables(nb, W, dtype=np.float32):
    """the tables the Viterbi launch reads, for a band of any width"""
    k = np.arange(2 * W + 1, dtype=np.float64)
    return dict(nb=nb, W=W, tri=np.log((W + 1.0 - np.abs(k - W)) / (W + 1.0) ** 2).astype(dtype), la=np.log(np.array([[0.99, 0.01], [0.01, 0.99]])).astype(dtype),
                f_bin=(71.0 * 2.0 ** (np.arange(nb) / 60.0)).astype(dtype))


@functools.lru_cache(maxsize=None)
def viterbi_case(nb, W, T, kind):
    """float32 (lv [T, nb], lu [T], bf0 [T, nb]) of a case.  'noise': log-probabilities of random masses, a tenth of lv at ln FLOOR.  'track': a planted
    voiced track that moves at most W bins per frame with an unvoiced stretch in the middle, over a background at ln FLOOR."""
    rng = np.random.RandomState(1000 * nb + 10 * W + T + (0 if kind == "noise" else 500000))
    low = np.float32(np.log(FLOOR))
    if kind == "noise":
        lv = np.log(rng.uniform(1e-6, 1.0, (T, nb))).astype(np.float32)
        lv[rng.rand(T, nb) < 0.1] = low
        lu = np.log(rng.uniform(1e-4, 1.0, T) / nb).astype(np.float32)
    else:
        lv = np.full((T, nb), low, dtype=np.float32)
        lu = np.full(T, np.float32(np.log(0.02 / nb)), dtype=np.float32)
        b = int(rng.randint(nb))
        for t in range(T):
            b = int(np.clip(b + rng.randint(-W, W + 1), 0, nb - 1))
            if T >= 6 and T // 3 <= t < T // 2:
                lu[t] = np.float32(np.log(0.98 / nb))
            else:
                lv[t, b] = np.float32(np.log(0.9))
                lv[t, rng.randint(nb)] = np.float32(np.log(0.05))
    bf0 = np.where(rng.rand(T, nb) < 0.5, rng.uniform(60.0, 900.0, (T, nb)), 0.0).astype(np.float32)
    for a in (lv, lu, bf0):
        a.setflags(write=False)
    return lv, lu, bf0


def tie_cases():
    """hand-made float32 inputs on which every comparison ties: [(name, nb, W, lv, lu)].  Constant rows: all bins carry the same V in every frame
    and the voiced and the unvoiced half mirror each other, in float32 as in float64, so only the rules decide -- the band's centre (tri's strict
    maximum), the same voicing (c1 > c0 is false on a tie), the lowest index at the end."""
    out = []
    for nb, W, T in ((1, 1, 4), (5, 2, 3), (5, 7, 4), (9, 3, 1)):
        out.append(("all equal nb %d W %d T %d" % (nb, W, T), nb, W, np.zeros((T, nb), dtype=np.float32), np.zeros(T, dtype=np.float32)))
    return out
