"""The forced-alignment contract of include/fcl_hip.h ("Forced alignment") restated in numpy: Gaussian log-likelihoods, the Viterbi
recurrence with its tie rules and backtrack, the statistics chain, the M-step, the flat-start trainer, and the synthetic corpus the tests fit.
Everything runs in float64 unless a dtype is passed; nothing here imports the package."""
import functools
import math

import numpy as np

U = 2.0 ** -24
T_MAX, S_MAX, D_MAX, M_MAX = 4096, 1024, 40, 1024
CHUNK = 8  # frames per staging chunk of al_viterbi_kernel (csrc/align.hip AL_CH)
VAR_FLOOR = 0.01


# ---- model ------------------------------------------------------------------------------------------------------------------------------------------
def gconst(var):
    """gconst[m] = -0.5 (D ln 2pi + sum_d ln var[m][d])"""
    var = np.asarray(var, dtype=np.float64)
    return -0.5 * (var.shape[1] * math.log(2.0 * math.pi) + np.log(var).sum(axis=1))


def params32(mean, var):
    """what the host uploads: mean, 1 / var and gconst, each formed in float64 and rounded to float32"""
    var = np.asarray(var, dtype=np.float64)
    return np.asarray(mean, dtype=np.float64).astype(np.float32), (1.0 / var).astype(np.float32), gconst(var).astype(np.float32)


def loglik(x, mean, ivar, gc):
    """float64 on the values given -> (ll [frames][M], q [frames][M])"""
    x, mean, ivar, gc = (np.asarray(v, dtype=np.float64) for v in (x, mean, ivar, gc))
    df = x[:, None, :] - mean[None, :, :]
    q = (df * df * ivar[None, :, :]).sum(axis=2)
    return gc[None, :] - 0.5 * q, q


def loglik_bound(q, ll, D):
    """The kernel rounds each difference once -- which its square carries twice --, the square once, and adds the D terms in one fma chain (D
    roundings at most on any term): every term of the non-negative sum q carries at most D + 3 factors (1 + delta), a relative error of at most
    gamma_(D + 3); the last fma rounds ll once.  The factor 1.01 covers the higher-order terms of (1 + u)^n."""
    return 1.01 * U * (0.5 * (D + 3) * np.asarray(q) + np.abs(ll))


# ---- utterance graph --------------------------------------------------------------------------------------------------------------------------------
def graph(phone_ids, optional, K):
    """phoneme indices and a flag per phoneme -> (row_state, row_skip, row_phone): K rows per phoneme, row_skip[a + K] = K + 1 behind an optional
    phoneme on the rows [a, a + K)"""
    n = len(phone_ids)
    row_state = np.asarray([p * K + k for p in phone_ids for k in range(K)], dtype=np.int32)
    row_phone = np.repeat(np.arange(n), K).astype(np.int32)
    row_skip = np.zeros(n * K, dtype=np.int32)
    for i, opt in enumerate(optional):
        if opt:
            assert 0 < i < n - 1 and not optional[i - 1] and not optional[i + 1]
            row_skip[(i + 1) * K] = K + 1
    return row_state, row_skip, row_phone


def optional_rows(row_skip):
    """the rows a skip jumps over"""
    opt = np.zeros(len(row_skip), dtype=bool)
    for r, j in enumerate(row_skip):
        if j >= 2:
            opt[r - j + 1 : r] = True
    return opt


def uniform_alignment(T, row_skip):
    """row_frames [S] of the equal split of T frames: over all rows when T >= S, over the mandatory rows otherwise (None when even they do not fit);
    row i of n gets floor((i + 1) T / n) - floor(i T / n) frames"""
    S = len(row_skip)
    opt = optional_rows(row_skip)
    rows = np.arange(S) if T >= S else np.flatnonzero(~opt)
    n = len(rows)
    if T < n or n == 0:
        return None
    edges = (np.arange(n + 1, dtype=np.int64) * T) // n
    out = np.zeros(S, dtype=np.int64)
    out[rows] = np.diff(edges)
    return out


# ---- Viterbi ----------------------------------------------------------------------------------------------------------------------------------------
def _backtrack(bp, row_skip, score, frame0):
    T, S = bp.shape
    frame_row = np.empty(T, dtype=np.int64)
    r = S - 1
    for t in range(T - 1, -1, -1):
        frame_row[t] = r
        if t > 0:
            r -= (0, 1, int(row_skip[r]))[bp[t, r]]
    if frame_row[0] != 0:
        return dict(ok=0, score=-np.inf, frame_row=np.full(T, -1, dtype=np.int64), row_begin=np.full(S, frame0, dtype=np.int64),
                    row_frames=np.zeros(S, dtype=np.int64))
    begin, count = runs(frame_row, S)
    return dict(ok=1, score=score, frame_row=frame_row, row_begin=begin + frame0, row_frames=count)


def runs(frame_row, S):
    """(row_begin, row_frames) of a non-decreasing frame_row: a row without frames begins where the next row with frames does"""
    T = len(frame_row)
    count = np.bincount(frame_row, minlength=S).astype(np.int64)
    begin = np.full(S, T, dtype=np.int64)
    nxt = T
    for r in range(S - 1, -1, -1):
        if count[r]:
            nxt = int(np.argmax(frame_row == r))
        begin[r] = nxt
    return begin, count


def _skip(row_skip):
    """a row_skip outside 2 .. 4 or pointing before row 0 counts as 0"""
    row_skip = np.asarray(row_skip, dtype=np.int64)
    r = np.arange(len(row_skip))
    return np.where((row_skip >= 2) & (row_skip <= 4) & (r - row_skip >= 0), row_skip, 0)


def viterbi_loop(ll, row_state, row_skip, dtype=np.float64, frame0=0):
    """the plain double loop over frames and rows, in `dtype` arithmetic"""
    ll = np.asarray(ll, dtype=dtype)
    T, S, skip = ll.shape[0], len(row_state), _skip(row_skip)
    ninf = dtype(-np.inf)
    V = np.full((T, S), ninf, dtype=dtype)
    bp = np.zeros((T, S), dtype=np.int8)
    V[0, 0] = ll[0, row_state[0]]
    for t in range(1, T):
        for r in range(S):
            best, mv = V[t - 1, r], 0
            if r > 0 and V[t - 1, r - 1] > best:
                best, mv = V[t - 1, r - 1], 1
            if skip[r] and V[t - 1, r - skip[r]] > best:
                best, mv = V[t - 1, r - skip[r]], 2
            with np.errstate(invalid="ignore"):
                V[t, r] = dtype(ll[t, row_state[r]] + best)
            bp[t, r] = mv
    return _backtrack(bp, skip, V[T - 1, S - 1], frame0)


def viterbi(ll, row_state, row_skip, dtype=np.float64, frame0=0):
    """the same recurrence, one vector operation per frame"""
    ll = np.asarray(ll, dtype=dtype)
    row_state = np.asarray(row_state, dtype=np.int64)
    T, S, skip = ll.shape[0], len(row_state), _skip(row_skip)
    has = skip > 0
    src = np.where(has, np.arange(S) - skip, 0)
    V = np.full(S, -np.inf, dtype=dtype)
    V[0] = ll[0, row_state[0]]
    bp = np.zeros((T, S), dtype=np.int8)
    ninf = np.full(1, -np.inf, dtype=dtype)
    for t in range(1, T):
        with np.errstate(invalid="ignore"):
            best = V.copy()
            adv = np.concatenate([ninf, V[:-1]])
            m1 = adv > best
            best[m1] = adv[m1]
            sk = np.where(has, V[src], ninf[0]).astype(dtype)
            m2 = has & (sk > best)
            best[m2] = sk[m2]
            bp[t] = np.where(m2, 2, np.where(m1, 1, 0))
            V = (ll[t, row_state] + best).astype(dtype)
    return _backtrack(bp, skip, V[S - 1], frame0)


def path_valid(frame_row, row_skip):
    """monotone, only allowed moves, row 0 in frame 0, the last row in the last frame"""
    fr, skip = np.asarray(frame_row, dtype=np.int64), _skip(row_skip)
    if fr[0] != 0 or fr[-1] != len(row_skip) - 1:
        return False
    step = np.diff(fr)
    return bool(np.all((step == 0) | (step == 1) | ((step >= 2) & (step == skip[fr[1:]]))))


def path_score(ll, row_state, frame_row):
    """(float64 sum of ll along the path, sum of |ll| along it)"""
    v = np.asarray(ll, dtype=np.float64)[np.arange(len(frame_row)), np.asarray(row_state)[frame_row]]
    return float(v.sum()), float(np.abs(v).sum())


# ---- statistics and the M-step ------------------------------------------------------------------------------------------------------------------------
def state_lists(row_state, M):
    """(state_off [M + 1], state_rows): the batch's rows grouped by model state, ascending row index inside a group"""
    row_state = np.asarray(row_state, dtype=np.int64)
    order = np.argsort(row_state, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(row_state, minlength=M))])
    return off.astype(np.int32), order.astype(np.int32)


def stats_chain(x, row_begin, row_frames, state_off, state_rows, acc_n, acc_s, acc_q):
    """ADDS to acc_n / acc_s / acc_q in the contract's order: per (state, coefficient) one float64 chain from 0 over the rows in list order, frames
    ascending, then one add to the accumulator"""
    x = np.asarray(x)
    assert x.dtype == np.float32
    for m in range(len(state_off) - 1):
        s, q, n = np.zeros(x.shape[1]), np.zeros(x.shape[1]), 0
        for r in state_rows[state_off[m] : state_off[m + 1]]:
            for f in range(int(row_begin[r]), int(row_begin[r]) + int(row_frames[r])):
                v = x[f].astype(np.float64)
                s = s + v
                q = q + v * v
            n += int(row_frames[r])
        acc_s[m] += s
        acc_q[m] += q
        acc_n[m] += n


def mstep(n, s, q, mean, var, var_floor=VAR_FLOOR):
    """mean = s / n, var = max(q / n - mean^2, var_floor x global variance); a state with n < 2 keeps its parameters"""
    n, s, q = np.asarray(n, dtype=np.float64), np.asarray(s, dtype=np.float64), np.asarray(q, dtype=np.float64)
    N = n.sum()
    gmean = s.sum(axis=0) / N
    floor = var_floor * (q.sum(axis=0) / N - gmean * gmean)
    mean, var = np.array(mean, dtype=np.float64), np.array(var, dtype=np.float64)
    for m in np.flatnonzero(n >= 2):
        mean[m] = s[m] / n[m]
        var[m] = np.maximum(q[m] / n[m] - mean[m] * mean[m], floor)
    return mean, var


def global_model(n, s, q, M):
    N = float(np.sum(n))
    gmean = np.sum(s, axis=0) / N
    gvar = np.sum(q, axis=0) / N - gmean * gmean
    return np.tile(gmean, (M, 1)), np.tile(gvar, (M, 1))


def _accumulate(feats, graphs, counts, M):
    D = feats[0].shape[1]
    n, s, q = np.zeros(M), np.zeros((M, D)), np.zeros((M, D))
    for x, (row_state, _), c in zip(feats, graphs, counts):
        if c is None:
            continue
        x = np.asarray(x, dtype=np.float64)
        edges = np.concatenate([[0], np.cumsum(c)])
        for r, m in enumerate(row_state):
            seg = x[edges[r] : edges[r + 1]]
            n[m] += len(seg)
            s[m] += seg.sum(axis=0)
            q[m] += (seg * seg).sum(axis=0)
    return n, s, q


def align(feats, graphs, mean, var):
    """float64 alignment of every utterance -> (row_frames or None per utterance, mean score per aligned frame)"""
    ivar, gc = 1.0 / var, gconst(var)
    counts, total, frames = [], 0.0, 0
    for x, (row_state, row_skip) in zip(feats, graphs):
        res = viterbi(loglik(x, mean, ivar, gc)[0], row_state, row_skip)
        counts.append(res["row_frames"] if res["ok"] else None)
        if res["ok"]:
            total, frames = total + float(res["score"]), frames + len(x)
    return counts, total / max(frames, 1)


def fit(feats, graphs, M, iterations, var_floor=VAR_FLOOR, callback=None):
    """The flat start: the statistics of the equal split give the first model (from the global mean and variance); then `iterations` times align
    and re-estimate.  -> (mean, var, the mean score per frame of each iteration)"""
    flat = [uniform_alignment(len(x), g[1]) for x, g in zip(feats, graphs)]
    n, s, q = _accumulate(feats, graphs, flat, M)
    mean, var = mstep(n, s, q, *global_model(n, s, q, M), var_floor=var_floor)
    history = []
    for it in range(iterations):
        counts, score = align(feats, graphs, mean, var)
        history.append(score)
        mean, var = mstep(*_accumulate(feats, graphs, counts, M), mean, var, var_floor=var_floor)
        if callback is not None:
            callback(it, mean, var)
    return mean, var, history


# ---- the synthetic corpus -----------------------------------------------------------------------------------------------------------------------------
N_PHONES, PAUSE = 12, 12  # the inventory: 12 phonemes and the pause, index 12


@functools.lru_cache(maxsize=None)
def corpus(seed, n_utt=60, K=3, D=8):
    """n_utt utterances of 6 .. 13 phonemes, K states of 2 .. 6 frames each, state means N(0, 2^2) and unit noise.  A pause follows half of the
    non-final phonemes in the transcript as an optional phoneme and is absent from 30 % of the recordings of it.
    -> dict(feats [x float32 [T, D]], graphs [(row_state, row_skip)], row_phone, truth [the transcript position of each frame], M, K)"""
    rng = np.random.RandomState(1000 + seed)
    M = (N_PHONES + 1) * K
    means = rng.randn(M, D) * 2.0
    feats, graphs, row_phones, truth = [], [], [], []
    for _ in range(n_utt):
        phones, optional = [], []
        n = rng.randint(6, 14)
        for i in range(n):
            phones.append(int(rng.randint(N_PHONES)))
            optional.append(False)
            if i < n - 1 and rng.rand() < 0.5:
                phones.append(PAUSE)
                optional.append(True)
        rows, pos = [], []
        for i, (p, opt) in enumerate(zip(phones, optional)):
            if opt and rng.rand() < 0.3:
                continue
            for k in range(K):
                d = int(rng.randint(2, 7))
                rows += [p * K + k] * d
                pos += [i] * d
        x = means[rows] + rng.randn(len(rows), D)
        row_state, row_skip, row_phone = graph(phones, optional, K)
        feats.append(x.astype(np.float32))
        graphs.append((row_state, row_skip))
        row_phones.append(row_phone)
        truth.append(np.asarray(pos))
    return dict(feats=feats, graphs=graphs, row_phone=row_phones, truth=truth, M=M, K=K, D=D)


def frame_accuracy(counts, row_phones, truth):
    """the share of frames whose aligned transcript position is the true one (an utterance without an alignment counts as all wrong)"""
    good = total = 0
    for c, rp, tr in zip(counts, row_phones, truth):
        total += len(tr)
        if c is not None:
            good += int((np.repeat(rp, c) == tr).sum())
    return good / float(total)


# ---- the inputs of the GPU Viterbi cases ----------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (1, 7), (3, 3), (3, 2), (9, 6), (9, 8), (9, 9), (255, 300), (256, 256), (257, 511), (1024, 1024), (1024, 4096),
         (5, CHUNK - 1), (5, CHUNK), (5, CHUNK + 1)]
KINDS = ("noise", "planted")


def case_graph(S):
    """one state per row (M = S); the 9-row cases have three phonemes of three states, the middle one optional; the large ones an optional
    three-row phoneme every 30 rows"""
    row_skip = np.zeros(S, dtype=np.int32)
    if S == 9:
        row_skip[6] = 4
    elif S >= 255:
        row_skip[33 : S - 3 : 30] = 4
    return np.arange(S, dtype=np.int32), row_skip


@functools.lru_cache(maxsize=None)
def case_ll(S, T, kind):
    """float32 ll [T][S]: Gaussian noise, or noise plus 8 on the cells of a planted segmentation (the equal split)"""
    rng = np.random.RandomState(S * 7 + T + len(kind))
    ll = (rng.randn(T, S) * 2.0 - 30.0).astype(np.float32)
    if kind == "planted":
        c = uniform_alignment(T, case_graph(S)[1])
        if c is not None:
            ll[np.arange(T), np.repeat(np.arange(S), c)] += np.float32(8.0)
    return ll


def exact_case(S, T, K, seed):
    """integer features and means with |v| <= 16, D = 4, ivar 1, gconst 0, T <= 40: every ll value -0.5 q is a multiple of 0.5 of at most 2^11 and
    every path sum one below 2^17, exact in float32 -> (ll float32 [T][M], row_state, row_skip)"""
    rng = np.random.RandomState(seed)
    n_ph = S // K
    assert n_ph * K == S and T <= 40
    D, M = 4, 5 * K
    mean = rng.randint(-16, 17, (M, D)).astype(np.float64)
    x = rng.randint(-16, 17, (T, D)).astype(np.float64)
    phones = list(rng.randint(0, 5, n_ph))
    optional = [0 < i < n_ph - 1 and i % 2 == 1 and rng.rand() < 0.7 for i in range(n_ph)]
    row_state, row_skip, _ = graph(phones, optional, K)
    ll = loglik(x, mean, np.ones((M, D)), np.zeros(M))[0]
    assert np.array_equal(ll.astype(np.float32).astype(np.float64), ll)
    return ll.astype(np.float32), row_state, row_skip
