"""The mixture entries of the forced-alignment contract (include/fcl_hip.h "Forced alignment, Gaussian-mixture states") restated in
float64 numpy: the clamp of comp_off, mixture log-likelihoods with their bound, component posteriors with theirs, the statistics chain, the split
rule, the M-step, the float64 trainer and the synthetic corpus with voices.  Nothing here imports the package; the single-Gaussian half is
tests/align_ref.py."""
import functools
import math

import numpy as np

import align_ref as R

U = R.U
C_MAX, G_MAX = 8, 8192
WEIGHT_FLOOR, SPLIT = 1e-5, 0.2
# The function errors of the device's expf and logf in ulp, the one thing rounding analysis cannot give.  The ROCm installation states no bound, so
# they were measured once on MI355X (tools/probe/al_gmm_ulp.hip: expf on [-87.3, 0], logf on [1, 8], the only arguments the kernels pass) against
# float64 at 4 M points each: worst 0.85 ulp (expf) and 2.31 ulp (logf); expf(0) is exactly 1 and logf(1) exactly 0.  The constants are twice the
# worst, rounded up to a power of two (DESIGN 6m's rule); they were fixed before any kernel of csrc/align_gmm.hip had run.
K_EXP, K_LOG = 2.0, 8.0


# ---- model ------------------------------------------------------------------------------------------------------------------------------------------
def params32(mean, var, weight):
    """what the host uploads: mean [G][D], 1 / var and cconst = ln w + gconst(var), formed in float64 and rounded to float32"""
    var = np.asarray(var, dtype=np.float64)
    cc = np.log(np.asarray(weight, dtype=np.float64)) + R.gconst(var)
    return np.asarray(mean, dtype=np.float64).astype(np.float32), (1.0 / var).astype(np.float32), cc.astype(np.float32)


def state_comps(comp_off, G, max_comp=C_MAX):
    """(g0 [M], cnt [M]) as the kernels read a comp_off they cannot trust: g0 = clamp(comp_off[m], 0, G - 1),
    cnt = clamp(comp_off[m + 1] - g0, 1, min(max_comp, G - g0))"""
    off = np.asarray(comp_off, dtype=np.int64)
    g0 = np.clip(off[:-1], 0, G - 1)
    return g0, np.maximum(np.minimum(off[1:] - g0, np.minimum(max_comp, G - g0)), 1)


def comp_loglik(x, mean, ivar, cc):
    """float64 on the values given -> (l [frames][G], q [frames][G]); align_ref.loglik one coefficient at a time (G may be 8192: no [frames][G][D])"""
    x, mean, ivar, cc = (np.asarray(v, dtype=np.float64) for v in (x, mean, ivar, cc))
    q = np.zeros((x.shape[0], mean.shape[0]))
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(x.shape[1]):
            df = x[:, d, None] - mean[None, :, d]
            q += df * df * ivar[None, :, d]
        return cc[None, :] - 0.5 * q, q


def _lse(v):
    """the contract's logsumexp over the last axis: a NaN wins the max; a non-finite max is the value"""
    with np.errstate(invalid="ignore", over="ignore"):
        mx = np.max(v, axis=-1)  # np.max propagates NaN
        ok = np.isfinite(mx)
        s = np.exp(v - np.where(ok, mx, 0.0)[..., None]).sum(axis=-1)
        return np.where(ok, mx + np.log(np.where(ok, s, 1.0)), mx)


def gmm_loglik(l, comp_off, max_comp=C_MAX):
    """l [frames][G] -> ll [frames][M]: a one-component state is l_0 itself, the others the logsumexp of their components"""
    l = np.asarray(l, dtype=np.float64)
    g0, cnt = state_comps(comp_off, l.shape[1], max_comp)
    out = np.empty((l.shape[0], len(g0)))
    for c in np.unique(cnt):
        ms = np.flatnonzero(cnt == c)
        v = l[:, g0[ms][:, None] + np.arange(c)[None, :]]  # [frames][states][c]
        out[:, ms] = v[:, :, 0] if c == 1 else _lse(v)
    return out


def gmm_loglik_loop(l, comp_off, max_comp=C_MAX):
    """the plain loop over frames, states and components"""
    l = np.asarray(l, dtype=np.float64)
    g0, cnt = state_comps(comp_off, l.shape[1], max_comp)
    out = np.empty((l.shape[0], len(g0)))
    for f in range(l.shape[0]):
        for m in range(len(g0)):
            v = [l[f, g0[m] + c] for c in range(cnt[m])]
            mx = v[0]
            for a in v[1:]:
                mx = a if (a > mx or a != a) else mx
            if cnt[m] == 1 or not math.isfinite(mx):
                out[f, m] = mx
                continue
            s = 0.0
            for a in v:
                s += math.exp(a - mx)
            out[f, m] = mx + math.log(s)
    return out


def kappa(C):
    """The roundings of the logsumexp of C >= 2 values beyond those of its arguments, in units of U = 2^-24, against a sum that is at least 1 (the
    dominant term is expf(0) = 1): each difference l_c - mx rounds once, which moves expf by e^a |a| U <= 0.37 U (C - 1 terms, the dominant one is
    exact); expf is off by K_EXP ulp <= 2 K_EXP U relative; the C - 1 additions round once each: the sum is off by (1.37 (C - 1) + 2 K_EXP) U
    relative, and ln moves by as much absolutely.  logf is off by K_LOG ulp of a value below ln 8 < 4: 4 K_LOG U.  (The last addition's U |ll| is
    the bound's own term.)"""
    return 1.37 * (C - 1) + 2.0 * K_EXP + 4.0 * K_LOG


def gmm_loglik_bound(q, l, ll, comp_off, D, max_comp=C_MAX):
    """[frames][M]: logsumexp moves by at most the largest perturbation of its arguments, so the first term is max_c loglik_bound(q_c, l_c, D);
    a state of C >= 2 components adds 1.01 U (kappa(C) + |ll|)"""
    b = R.loglik_bound(q, l, D)
    g0, cnt = state_comps(comp_off, np.shape(l)[1], max_comp)
    out = np.empty(np.shape(ll))
    for m in range(len(g0)):
        out[:, m] = b[:, g0[m] : g0[m] + cnt[m]].max(axis=1)
        if cnt[m] > 1:
            out[:, m] += 1.01 * U * (kappa(cnt[m]) + np.abs(ll[:, m]))
    return out


# ---- posteriors ---------------------------------------------------------------------------------------------------------------------------------------
def frame_states(row_state, row_begin, row_frames, frames):
    """frame_state [frames]: the model state of the row each frame belongs to, -1 where no row has it (an utterance without an alignment)"""
    out = np.full(frames, -1, dtype=np.int32)
    for r in range(len(row_state)):
        out[int(row_begin[r]) : int(row_begin[r]) + int(row_frames[r])] = row_state[r]
    return out


def posteriors(l, comp_off, frame_state, max_comp=C_MAX):
    """l [frames][G] float64 -> (gamma [frames][8], arg [frames][8] = l_c - mx, cnt [frames]): exactly 1 for a one-component state, 0 beyond the
    state's count and for a negative frame_state; frame_state above M - 1 counts as M - 1"""
    l = np.asarray(l, dtype=np.float64)
    g0, cnt = state_comps(comp_off, l.shape[1], max_comp)
    fs = np.asarray(frame_state, dtype=np.int64)
    m = np.clip(fs, 0, len(g0) - 1)
    k = np.arange(C_MAX)[None, :]
    mask = k < cnt[m][:, None]
    v = np.where(mask, l[np.arange(len(m))[:, None], np.minimum(g0[m][:, None] + k, l.shape[1] - 1)], -np.inf)
    arg = v - v.max(axis=1, keepdims=True)
    e = np.where(mask, np.exp(arg), 0.0)
    gamma = e / e.sum(axis=1, keepdims=True)
    gamma[cnt[m] == 1] = np.eye(C_MAX)[0]
    gamma[fs < 0] = 0.0
    return gamma, np.where(mask, arg, 0.0), np.where(fs < 0, 0, cnt[m])


def posterior_bound(gamma, arg, cnt, B):
    """ln gamma_c = l_c - ln sum_k e^(l_k) moves by at most 2 B when every l moves by at most B (B [frames]: the largest l_c bound of the frame's
    state).  The roundings: the difference once (U |arg_c| on the exponent), expf 2 K_EXP U, the sum (1.37 (C - 1) + 2 K_EXP) U as in kappa, the
    division once; 2^-126 absolutely for a quotient below the normal range.  All relative to gamma; 1.01 for the higher orders."""
    C = np.asarray(cnt, dtype=np.float64)[:, None]
    return 1.01 * gamma * (2.0 * np.asarray(B)[:, None] + U * (np.abs(arg) + 4.0 * K_EXP + 1.37 * np.maximum(C - 1.0, 0.0) + 1.0)) + 2.0 ** -126


# ---- statistics ---------------------------------------------------------------------------------------------------------------------------------------
def stats_chain(x, gamma, row_begin, row_frames, state_off, state_rows, comp_off, acc_w, acc_s, acc_q, max_comp=C_MAX):
    """ADDS to acc_w [G] / acc_s / acc_q [G][D] in the contract's order: per (component, coefficient) one float64 chain from 0 over the state's rows
    in list order, frames ascending -- g = (double)gamma, v = (double)x, p = g v, w += g, s += p, q += p v, every product and sum rounded on its own
    (numpy fuses nothing) -- then one add to the accumulator"""
    x, gamma = np.asarray(x), np.asarray(gamma)
    assert x.dtype == np.float32 and gamma.dtype == np.float32 and gamma.shape[1] == C_MAX
    g0, cnt = state_comps(comp_off, len(acc_w), max_comp)
    for m in range(len(state_off) - 1):
        C = int(cnt[m])
        w, s, q = np.zeros(C), np.zeros((C, x.shape[1])), np.zeros((C, x.shape[1]))
        for r in state_rows[state_off[m] : state_off[m + 1]]:
            for f in range(int(row_begin[r]), int(row_begin[r]) + int(row_frames[r])):
                g, v = gamma[f, :C].astype(np.float64), x[f].astype(np.float64)
                p = g[:, None] * v[None, :]
                w = w + g
                s = s + p
                q = q + p * v[None, :]
        acc_w[g0[m] : g0[m] + C] += w
        acc_s[g0[m] : g0[m] + C] += s
        acc_q[g0[m] : g0[m] + C] += q


# ---- split and M-step -----------------------------------------------------------------------------------------------------------------------------------
def split_to(mean, var, weight, occ, comp_off, target, min_occupancy):
    """Per state, while it has fewer than `target` components: take the component of largest weight (the first on ties); stop for this state if its
    occupancy is below 2 min_occupancy; otherwise halve its weight and occupancy, move it to mean + 0.2 sigma and append a copy at mean - 0.2 sigma
    with the same variance at the end of the state's list.  -> (mean, var, weight, occ, comp_off) of the grown model"""
    mean, var, weight, occ = (np.asarray(v, dtype=np.float64) for v in (mean, var, weight, occ))
    out_m, out_v, out_w, out_o, off = [], [], [], [], [0]
    for m in range(len(comp_off) - 1):
        sl = slice(int(comp_off[m]), int(comp_off[m + 1]))
        mu, va, w, o = [r.copy() for r in mean[sl]], [r.copy() for r in var[sl]], list(weight[sl]), list(occ[sl])
        while len(w) < target:
            j = int(np.argmax(w))  # the first of equal weights
            if o[j] < 2.0 * min_occupancy:
                break
            w[j], o[j] = w[j] / 2.0, o[j] / 2.0
            step = SPLIT * np.sqrt(va[j])
            mu.append(mu[j] - step)
            va.append(va[j].copy())
            w.append(w[j])
            o.append(o[j])
            mu[j] = mu[j] + step
        out_m += mu
        out_v += va
        out_w += w
        out_o += o
        off.append(len(out_w))
    return np.asarray(out_m), np.asarray(out_v), np.asarray(out_w), np.asarray(out_o), np.asarray(off, dtype=np.int32)


def targets(mixtures):
    """2, 4, ... and the last target is `mixtures` itself"""
    out, t = [], 2
    while t < mixtures:
        out.append(t)
        t *= 2
    return out + ([int(mixtures)] if mixtures > 1 else [])


def mstep(w, s, q, mean, var, weight, comp_off, var_floor=R.VAR_FLOOR):
    """a component with acc_w >= 2: mean = s / w, var = max(q / w - mean^2, var_floor x the global variance of this pass), the others keep their
    parameters; a state with occupancy >= 2: weights max(acc_w / occupancy, 1e-5), renormalised"""
    w, s, q = (np.asarray(v, dtype=np.float64) for v in (w, s, q))
    N = w.sum()
    gmean = s.sum(axis=0) / N
    floor = var_floor * (q.sum(axis=0) / N - gmean * gmean)
    mean, var, weight = np.array(mean, dtype=np.float64), np.array(var, dtype=np.float64), np.array(weight, dtype=np.float64)
    for g in np.flatnonzero(w >= 2):
        mean[g] = s[g] / w[g]
        var[g] = np.maximum(q[g] / w[g] - mean[g] * mean[g], floor)
    for m in range(len(comp_off) - 1):
        sl = slice(int(comp_off[m]), int(comp_off[m + 1]))
        occ = w[sl].sum()
        if occ >= 2:
            v = np.maximum(w[sl] / occ, WEIGHT_FLOOR)
            weight[sl] = v / v.sum()
    return mean, var, weight


# ---- the float64 trainer ----------------------------------------------------------------------------------------------------------------------------------
def viterbi_batch(lls, graphs):
    """align_ref.viterbi on every utterance at once (the trainer aligns 120 utterances 17 times): the same float64 recurrence with the same tie
    rules, one vector operation per frame over [utterances][rows]; rows past an utterance's own hold -inf, an utterance past its last frame keeps
    its column.  -> what align_ref.viterbi returns, per utterance"""
    n, S, T = len(lls), [len(g[0]) for g in graphs], [len(l) for l in lls]
    Sm, Tm, Tn = max(S), max(T), np.asarray([len(l) for l in lls])
    skip = np.zeros((n, Sm), dtype=np.int64)
    E = np.full((n, Tm, Sm), -np.inf)
    for u, (ll, (row_state, row_skip)) in enumerate(zip(lls, graphs)):
        skip[u, : S[u]] = R._skip(row_skip)
        E[u, : T[u], : S[u]] = np.asarray(ll, dtype=np.float64)[:, np.asarray(row_state, dtype=np.int64)]
    has, rows = skip > 0, np.arange(n)[:, None]
    src = np.where(has, np.arange(Sm)[None, :] - skip, 0)
    V = np.full((n, Sm), -np.inf)
    V[:, 0] = E[:, 0, 0]
    bp = np.zeros((n, Tm, Sm), dtype=np.int8)
    ninf = np.full((n, 1), -np.inf)
    with np.errstate(invalid="ignore"):
        for t in range(1, Tm):
            best = V.copy()
            adv = np.concatenate([ninf, V[:, :-1]], axis=1)
            m1 = adv > best
            best[m1] = adv[m1]
            sk = np.where(has, V[rows, src], -np.inf)
            m2 = has & (sk > best)
            best[m2] = sk[m2]
            bp[:, t] = np.where(m2, 2, np.where(m1, 1, 0))
            V = np.where((t < Tn)[:, None], E[:, t] + best, V)
    return [R._backtrack(bp[u, : T[u], : S[u]], skip[u, : S[u]], V[u, S[u] - 1], 0) for u in range(n)]


def align(feats, graphs, mean, var, weight, comp_off):
    """float64 alignment with the mixtures -> (row_frames or None per utterance, the component values l per utterance)"""
    ivar, cc = 1.0 / var, np.log(weight) + R.gconst(var)
    ls = [comp_loglik(x, mean, ivar, cc)[0] for x in feats]
    res = viterbi_batch([gmm_loglik(l, comp_off) for l in ls], graphs)
    return [r["row_frames"] if r["ok"] else None for r in res], ls


def accumulate(feats, graphs, counts, ls, comp_off, G):
    """the soft statistics of an alignment, vectorised: the posteriors of every frame inside the state the path gave it"""
    D = feats[0].shape[1]
    w, s, q = np.zeros(G), np.zeros((G, D)), np.zeros((G, D))
    g0, cnt = state_comps(comp_off, G)
    k = np.arange(C_MAX)[None, :]
    for x, (row_state, _), c, l in zip(feats, graphs, counts, ls):
        if c is None:
            continue
        fs = np.repeat(row_state, c)
        gamma = posteriors(l, comp_off, fs)[0]
        mask = k < cnt[fs][:, None]
        idx = (g0[fs][:, None] + k)[mask]
        fr = np.broadcast_to(np.arange(len(fs))[:, None], mask.shape)[mask]
        g, v = gamma[mask], np.asarray(x, dtype=np.float64)[fr]
        np.add.at(w, idx, g)
        np.add.at(s, idx, g[:, None] * v)
        np.add.at(q, idx, g[:, None] * v * v)
    return w, s, q


def fit(feats, graphs, M, iterations, mixtures=1, mix_iterations=4, min_occupancy=10.0, var_floor=R.VAR_FLOOR, callback=None):
    """align_ref.fit's single-Gaussian stage, then for every target: split, and mix_iterations times align and re-estimate.
    -> dict(mean, var, weight, comp_off, components: the component total of every round).  callback(stage, model) runs after the single-Gaussian
    stage (stage 1) and after the rounds of every target (stage = the target)."""
    flat = [R.uniform_alignment(len(x), g[1]) for x, g in zip(feats, graphs)]
    n, s, q = R._accumulate(feats, graphs, flat, M)
    mean, var = R.mstep(n, s, q, *R.global_model(n, s, q, M), var_floor=var_floor)
    components = []
    one = np.arange(M + 1, dtype=np.int32)
    for _ in range(iterations):
        counts, _ = align(feats, graphs, mean, var, np.ones(M), one)  # one component of weight 1: align_ref.align's alignment
        n, s, q = R._accumulate(feats, graphs, counts, M)
        mean, var = R.mstep(n, s, q, mean, var, var_floor=var_floor)
        components.append(M)
    weight, occ, comp_off = np.ones(M), np.asarray(n, dtype=np.float64), np.arange(M + 1, dtype=np.int32)
    model = dict(mean=mean, var=var, weight=weight, comp_off=comp_off)
    if callback is not None:
        callback(1, model)
    for target in targets(mixtures):
        mean, var, weight, occ, comp_off = split_to(mean, var, weight, occ, comp_off, target, min_occupancy)
        for _ in range(mix_iterations):
            counts, ls = align(feats, graphs, mean, var, weight, comp_off)
            w, s, q = accumulate(feats, graphs, counts, ls, comp_off, len(weight))
            mean, var, weight = mstep(w, s, q, mean, var, weight, comp_off, var_floor=var_floor)
            occ = w
            components.append(len(weight))
        model = dict(mean=mean, var=var, weight=weight, comp_off=comp_off)
        if callback is not None:
            callback(target, model)
    model["components"] = components
    return model


# ---- the synthetic corpus with voices -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def corpus_voices(seed, n_utt=120, K=3, D=4, sep=1.0, mode=3.0, voices=3):
    """align_ref.corpus with voices: every state's mean is shifted by one of `voices` offsets N(0, mode^2), the voice drawn per utterance -- a state's
    realisations fall into `voices` clusters, which one Gaussian can only cover with its variance"""
    rng = np.random.RandomState(2000 + seed)
    M = (R.N_PHONES + 1) * K
    means = rng.randn(M, D) * sep
    shift = rng.randn(voices, M, D) * mode
    feats, graphs, row_phones, truth = [], [], [], []
    for _ in range(n_utt):
        v = int(rng.randint(voices))
        phones, optional = [], []
        n = rng.randint(6, 14)
        for i in range(n):
            phones.append(int(rng.randint(R.N_PHONES)))
            optional.append(False)
            if i < n - 1 and rng.rand() < 0.5:
                phones.append(R.PAUSE)
                optional.append(True)
        rows, pos = [], []
        for i, (p, opt) in enumerate(zip(phones, optional)):
            if opt and rng.rand() < 0.3:
                continue
            for k in range(K):
                d = int(rng.randint(2, 7))
                rows += [p * K + k] * d
                pos += [i] * d
        x = means[rows] + shift[v][rows] + rng.randn(len(rows), D)
        row_state, row_skip, row_phone = R.graph(phones, optional, K)
        feats.append(x.astype(np.float32))
        graphs.append((row_state, row_skip))
        row_phones.append(row_phone)
        truth.append(np.asarray(pos))
    return dict(feats=feats, graphs=graphs, row_phone=row_phones, truth=truth, M=M, K=K, D=D)


SCHEDULE = dict(iterations=6, mixtures=4, mix_iterations=4, min_occupancy=10.0)


@functools.lru_cache(maxsize=None)
def fit_voices(seed):
    """the float64 trainer on corpus_voices(seed) with SCHEDULE -> (frame accuracy of the single-Gaussian stage, of 2 and of 4 components, the model)"""
    c = corpus_voices(seed)
    acc = {}

    def check(stage, m):
        counts, _ = align(c["feats"], c["graphs"], m["mean"], m["var"], m["weight"], m["comp_off"])
        acc[stage] = R.frame_accuracy(counts, c["row_phone"], c["truth"])

    model = fit(c["feats"], c["graphs"], c["M"], callback=check, **SCHEDULE)
    return acc[1], acc[2], acc[4], model
