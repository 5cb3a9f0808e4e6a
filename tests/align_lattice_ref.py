"""The lattice Viterbi contract of include/fcl_hip.h ("Forced alignment, lattice graphs") restated in numpy: the recurrence over rows
with up to 8 predecessor slots and START / FINAL flags, its tie rules, the choice of the end row and the backtrack; a chain written as a lattice; the
word graph; a brute-force enumerator of all valid paths for tiny lattices; the inputs of the GPU kernel cases; the flat-start trainer over word
graphs and the synthetic word corpus it fits.  float64 unless a dtype is passed; nothing here imports the package."""
import functools

import numpy as np

import align_ref as R

SLOTS, START, FINAL = 8, 1, 2


# ---- the recurrence ---------------------------------------------------------------------------------------------------------------------------------
def usable(row_pred):
    """[S][8] int64: the slot values that count (j >= 1 and r - j >= 0), 0 elsewhere"""
    p = np.asarray(row_pred, dtype=np.int64).reshape(-1, SLOTS)
    r = np.arange(len(p))[:, None]
    return np.where((p >= 1) & (r - p >= 0), p, 0)


def _failed(T, S, frame0):
    return dict(ok=0, score=-np.inf, frame_row=np.full(T, -1, dtype=np.int64), row_begin=np.full(S, frame0, dtype=np.int64),
                row_frames=np.zeros(S, dtype=np.int64))


def runs(frame_row, S, frame0=0):
    """(row_begin, row_frames) of a non-decreasing frame_row: a row off the path has 0 frames and begins at the utterance's first frame"""
    count = np.bincount(frame_row, minlength=S).astype(np.int64)
    begin = np.full(S, frame0, dtype=np.int64)
    for r in np.flatnonzero(count):
        begin[r] = frame0 + int(np.argmax(frame_row == r))
    return begin, count


def lattice_viterbi(ll, row_state, row_pred, row_flags, dtype=np.float64, frame0=0):
    """V(r, 0) = ll(0, state r) on a START row, -inf elsewhere; V(r, t) = ll(t, state r) + best, best = stay, then the usable slots in slot order,
    each replacing the winner only when strictly greater; the end row is the FINAL row with the largest finite V(r, T - 1), the lowest on ties;
    the same loop in float64 and float32"""
    ll = np.asarray(ll, dtype=dtype)
    row_state = np.asarray(row_state, dtype=np.int64)
    T, S = ll.shape[0], len(row_state)
    pred, flags = usable(row_pred), np.asarray(row_flags, dtype=np.int64) & 3
    src = np.arange(S)[:, None] - pred
    slots = [s for s in range(SLOTS) if pred[:, s].any()]
    ninf = dtype(-np.inf)
    V = np.where(flags & START, ll[0, row_state], ninf).astype(dtype)
    bp = np.zeros((T, S), dtype=np.int8)
    for t in range(1, T):
        with np.errstate(invalid="ignore"):
            best, mv = V.copy(), np.zeros(S, dtype=np.int8)
            for s in slots:
                c = V[src[:, s]]
                m = (pred[:, s] > 0) & (c > best)
                best[m], mv[m] = c[m], 1 + s
            V = (ll[t, row_state] + best).astype(dtype)
        bp[t] = mv
    final = np.flatnonzero(((flags & FINAL) > 0) & np.isfinite(V))
    if len(final) == 0:
        return _failed(T, S, frame0)
    r = int(final[np.argmax(V[final])])  # argmax: the first of equal values, the lowest row
    score = V[r]
    frame_row = np.empty(T, dtype=np.int64)
    for t in range(T - 1, -1, -1):
        frame_row[t] = r
        if t > 0 and bp[t, r]:
            r -= int(pred[r, bp[t, r] - 1])
    if not flags[frame_row[0]] & START:
        return _failed(T, S, frame0)
    begin, count = runs(frame_row, S, frame0)
    return dict(ok=1, score=score, frame_row=frame_row, row_begin=begin, row_frames=count)


def path_valid(frame_row, row_pred, row_flags):
    """a START row in frame 0, a FINAL row in the last frame, every move a stay or one of the row's usable slots"""
    fr, pred, flags = np.asarray(frame_row, dtype=np.int64), usable(row_pred), np.asarray(row_flags, dtype=np.int64)
    if fr.min() < 0 or fr.max() >= len(pred) or not flags[fr[0]] & START or not flags[fr[-1]] & FINAL:
        return False
    step = np.diff(fr)
    return bool(np.all((step == 0) | ((step > 0) & (pred[fr[1:]] == step[:, None]).any(axis=1))))


def chain_as_lattice(row_skip):
    """the chain of fcl_al_viterbi_fwd as a lattice: slot 0 = 1 on every row r > 0, slot 1 = row_skip[r] where usable, START on row 0, FINAL on the
    last row -> (row_pred, row_flags)"""
    S = len(row_skip)
    pred, flags = np.zeros((S, SLOTS), dtype=np.int32), np.zeros(S, dtype=np.int32)
    pred[1:, 0] = 1
    pred[:, 1] = R._skip(row_skip)
    flags[0] |= START
    flags[S - 1] |= FINAL
    return pred, flags


# ---- brute force ------------------------------------------------------------------------------------------------------------------------------------
def brute_force(ll, row_state, row_pred, row_flags):
    """Every valid path of a tiny lattice, scored in float64 (exact on integer-valued ll).  The tie rules of the recurrence, said globally: of the
    paths with the best score the one with the lowest end row; then, frame after frame from the end, the one whose move into that frame comes first
    in the order stay, slot 0, ..., slot 7 (a distance that several slots name belongs to the first of them).  -> dict(ok, score, frame_row)"""
    ll = np.asarray(ll, dtype=np.float64)
    T, S = ll.shape[0], len(row_state)
    pred, flags = usable(row_pred), np.asarray(row_flags, dtype=np.int64)
    moves = []  # per row: [(code, source row)] in the order of the tie rule
    for r in range(S):
        m, seen = [(0, r)], set()
        for s in range(SLOTS):
            d = int(pred[r, s])
            if d and d not in seen:
                seen.add(d)
                m.append((1 + s, r - d))
        moves.append(m)
    paths = []  # (score, key, frame_row): key = (end row, the move codes from the last frame backwards)

    def walk(t, r, rows, codes):
        if t == 0:
            if flags[r] & START:
                fr = rows[::-1]
                paths.append((sum(ll[i, row_state[q]] for i, q in enumerate(fr)), (fr[-1],) + tuple(codes), fr))
            return
        for code, src in moves[r]:
            walk(t - 1, src, rows + [src], codes + [code])

    for r in range(S):
        if flags[r] & FINAL:
            walk(T - 1, r, [r], [])
    if not paths:
        return dict(ok=0, score=-np.inf, frame_row=np.full(T, -1, dtype=np.int64), n_paths=0)
    best = max(p[0] for p in paths)
    tied = [p for p in paths if p[0] == best]
    win = min(tied, key=lambda p: p[1])
    return dict(ok=1, score=best, frame_row=np.asarray(win[2], dtype=np.int64), n_paths=len(paths), n_tied=len(tied))


def tiny_lattice(seed):
    """a seeded lattice of 1 .. 6 rows with integer-valued ll [T <= 6][3] in -3 .. 0, so that ties do occur: random slots (duplicates, zeros and
    unusable values among them), random START / FINAL rows"""
    rng = np.random.RandomState(seed)
    S, T = int(rng.randint(1, 7)), int(rng.randint(1, 7))
    pred = rng.randint(-1, 4, (S, SLOTS)).astype(np.int32) * (rng.rand(S, SLOTS) < 0.4)
    flags = (rng.rand(S) < 0.4) * START + (rng.rand(S) < 0.4) * FINAL
    flags[0] |= START
    if seed % 5:
        flags[S - 1] |= FINAL
    return rng.randint(-3, 1, (T, 3)).astype(np.float64), rng.randint(0, 3, S).astype(np.int32), pred.astype(np.int32), flags.astype(np.int32)


# ---- the word graph -----------------------------------------------------------------------------------------------------------------------------------
def word_graph(words, silence, K, boundary=True):
    """words: per word its variants, each a list of phoneme indices; silence: the phoneme index of the silence.  The layout
    [sil_0] w_0 [sil_1] w_1 ... w_(n-1) [sil_n]: a word is its variants' chains one after the other, a silence K rows; sil_0 / sil_n only with
    boundary.  Slot 0 = 1 on inner rows; the first row of sil_i (i >= 1) is entered from the last rows of the variants of w_(i-1) in variant order;
    the first row of a variant of w_i from the last row of sil_i (slot 0, when there is one), then from those of the variants of w_(i-1).
    -> dict(row_state, row_pred, row_flags, row_phone, row_word, row_variant)"""
    n = len(words)
    state, phone, word, variant, pred, flags = [], [], [], [], [], []

    def chain(labels, w, v, sources):
        first = len(state)
        for p in labels:
            for k in range(K):
                r = len(state)
                state.append(p * K + k), phone.append(p), word.append(w), variant.append(v), flags.append(0)
                slots = [1] if r > first else [r - s for s in sources]
                assert len(slots) <= SLOTS
                pred.append(slots + [0] * (SLOTS - len(slots)))
        return first, len(state) - 1

    ends = []
    for i in range(n + 1):
        sil = None
        if boundary or 0 < i < n:
            sil = chain([silence], -1, -1, ends)
            if i == 0:
                flags[sil[0]] |= START
            if i == n:
                flags[sil[1]] |= FINAL
        if i == n:
            break
        new = []
        for v, labels in enumerate(words[i]):
            first, last = chain(labels, i, v, ([sil[1]] if sil else []) + ends)
            if i == 0:
                flags[first] |= START
            if i == n - 1:
                flags[last] |= FINAL
            new.append(last)
        ends = new
    a = lambda v: np.asarray(v, dtype=np.int32)
    return dict(row_state=a(state), row_pred=a(pred).reshape(-1, SLOTS), row_flags=a(flags), row_phone=a(phone), row_word=a(word), row_variant=a(variant))


def canonical_rows(g, boundary=True):
    """the canonical chain: the first-listed variant of every word, with sil_0 and sil_n when boundary"""
    word = np.flatnonzero(g["row_word"] >= 0)
    keep = g["row_variant"] == 0
    if boundary:
        r = np.arange(len(g["row_word"]))
        keep = keep | ((g["row_word"] < 0) & ((r < word[0]) | (r > word[-1])))
    return np.flatnonzero(keep)


def uniform_alignment(T, g):
    """the flat start: the equal split over the canonical chain, without the two end silences when T is below its row count, None when that does
    not fit either; row i of the n rows taken gets floor((i + 1) T / n) - floor(i T / n) frames"""
    for boundary in (True, False):
        rows = canonical_rows(g, boundary)
        n = len(rows)
        if n and T >= n:
            out = np.zeros(len(g["row_state"]), dtype=np.int64)
            out[rows] = np.diff((np.arange(n + 1, dtype=np.int64) * T) // n)
            return out
    return None


def row_codes(g, K):
    """a code per row that says where in the utterance it stands, whatever the variant: 64 x slot + the label's position inside its variant, slot =
    2 i for sil_i and 2 i + 1 for w_i"""
    codes, last_word, first = np.zeros(len(g["row_word"]), dtype=np.int64), -1, {}
    for r, (w, v) in enumerate(zip(g["row_word"], g["row_variant"])):
        if w < 0:
            codes[r] = 64 * 2 * (last_word + 1)
        else:
            last_word = int(w)
            codes[r] = 64 * (2 * w + 1) + (r - first.setdefault((int(w), int(v)), r)) // K
    return codes


# ---- the trainer over word graphs -----------------------------------------------------------------------------------------------------------------------
def align(feats, graphs, mean, var):
    """float64 alignment of every utterance -> (row_frames or None per utterance, mean score per aligned frame)"""
    ivar, gc = 1.0 / var, R.gconst(var)
    counts, total, frames = [], 0.0, 0
    for x, g in zip(feats, graphs):
        res = lattice_viterbi(R.loglik(x, mean, ivar, gc)[0], g["row_state"], g["row_pred"], g["row_flags"])
        counts.append(res["row_frames"] if res["ok"] else None)
        if res["ok"]:
            total, frames = total + float(res["score"]), frames + len(x)
    return counts, total / max(frames, 1)


def fit(feats, graphs, M, iterations, var_floor=R.VAR_FLOOR):
    """align_ref.fit over word graphs: the flat start on the canonical chains (a state without statistics keeps the global model), then
    `iterations` times align and re-estimate.  The rows of a path ascend and the others have no frames, so the statistics of align_ref run
    unchanged.  -> (mean, var, the mean score per frame of each iteration)"""
    pairs = [(g["row_state"], None) for g in graphs]
    flat = [uniform_alignment(len(x), g) for x, g in zip(feats, graphs)]
    n, s, q = R._accumulate(feats, pairs, flat, M)
    mean, var = R.mstep(n, s, q, *R.global_model(n, s, q, M), var_floor=var_floor)
    history = []
    for _ in range(iterations):
        counts, score = align(feats, graphs, mean, var)
        history.append(score)
        mean, var = R.mstep(*R._accumulate(feats, pairs, counts, M), mean, var, var_floor=var_floor)
    return mean, var, history


def chosen_variants(g, row_frames):
    """per word the variant whose rows hold frames (-1: none)"""
    out = np.full(int(g["row_word"].max()) + 1, -1, dtype=np.int64)
    for r in np.flatnonzero(np.asarray(row_frames) > 0):
        if g["row_word"][r] >= 0:
            out[g["row_word"][r]] = g["row_variant"][r]
    return out


def variant_accuracy(counts, graphs, picks, vocab):
    """the share of the multi-variant words of the corpus that were given the variant the recording holds (an utterance without an alignment
    counts as all wrong)"""
    good = total = 0
    for c, g, (words, chosen) in zip(counts, graphs, picks):
        got = chosen_variants(g, c) if c is not None else None
        for i, (w, v) in enumerate(zip(words, chosen)):
            if len(vocab[w]) > 1:
                total += 1
                good += int(got is not None and got[i] == v)
    return good / float(max(total, 1)), total


# ---- the synthetic word corpus -----------------------------------------------------------------------------------------------------------------------
N_PHONES, SIL, N_WORDS = 12, 12, 20  # 12 phonemes and the silence, index 12; a vocabulary of 20 words


def vocabulary(rng):
    """20 words of 2 .. 4 phonemes; every third word has 2 .. 3 variants, each differing from the first in at least one phoneme"""
    vocab = []
    for w in range(N_WORDS):
        base = [int(p) for p in rng.randint(N_PHONES, size=rng.randint(2, 5))]
        variants = [base]
        if w % 3 == 0:
            while len(variants) < 1 + (1 + (w // 3) % 2):
                v = list(base)
                for pos in rng.choice(len(base), size=rng.randint(1, 3), replace=False):
                    v[pos] = int((v[pos] + 1 + rng.randint(N_PHONES - 1)) % N_PHONES)
                if v not in variants:
                    variants.append(v)
        vocab.append(variants)
    return vocab


@functools.lru_cache(maxsize=None)
def corpus(seed, n_utt=60, K=3, D=8):
    """n_utt utterances of 4 .. 9 words built like align_ref.corpus: K states of 2 .. 6 frames each, state means N(0, 2^2) and unit noise.  Every
    recording picks a variant of each word at random, has a leading and a trailing silence and a silence between two words half of the time.
    -> dict(feats, graphs (word_graph), codes (row_codes per utterance), truth (the code of each frame), picks [(word ids, chosen variants)],
    vocab, M, K, D)"""
    rng = np.random.RandomState(2000 + seed)
    M = (N_PHONES + 1) * K
    means = rng.randn(M, D) * 2.0
    vocab = vocabulary(rng)
    feats, graphs, codes, truth, picks = [], [], [], [], []
    for _ in range(n_utt):
        words = [int(w) for w in rng.randint(N_WORDS, size=rng.randint(4, 10))]
        chosen = [int(rng.randint(len(vocab[w]))) for w in words]
        rows, code = [], []

        def emit(p, c):
            for k in range(K):
                d = int(rng.randint(2, 7))
                rows.extend([p * K + k] * d)
                code.extend([c] * d)

        emit(SIL, 0)
        for i, (w, v) in enumerate(zip(words, chosen)):
            if i > 0 and rng.rand() < 0.5:
                emit(SIL, 64 * 2 * i)
            for pos, p in enumerate(vocab[w][v]):
                emit(p, 64 * (2 * i + 1) + pos)
        emit(SIL, 64 * 2 * len(words))
        g = word_graph([vocab[w] for w in words], SIL, K)
        feats.append((means[rows] + rng.randn(len(rows), D)).astype(np.float32))
        graphs.append(g)
        codes.append(row_codes(g, K))
        truth.append(np.asarray(code))
        picks.append((words, chosen))
    return dict(feats=feats, graphs=graphs, codes=codes, truth=truth, picks=picks, vocab=vocab, M=M, K=K, D=D)


# ---- the inputs of the GPU kernel cases -----------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (1, 7), (3, 2), (9, 6), (9, 9), (255, 300), (256, 256), (257, 511), (1024, 1024), (1024, 4096), (5, R.CHUNK - 1), (5, R.CHUNK),
         (5, R.CHUNK + 1)]
KINDS = ("chain", "words", "dense")


def fits(S, kind):
    """dense lattices need a row per START and FINAL flag of the four"""
    return kind != "dense" or S >= 5


@functools.lru_cache(maxsize=None)
def case_lattice(S, kind):
    """-> (row_state, row_pred, row_flags, M) of exactly S rows.  chain: align_ref.case_graph as a lattice.  words: a word_graph of random words
    with 1 .. 4 variants (20 phonemes and a silence; K = 3, 2 or 1, whichever divides S).  dense: 8 slots on every row at random distances in
    1 .. min(r, 300), 4 START and 4 FINAL rows, one state per row."""
    rng = np.random.RandomState(31 * S + len(kind))
    if kind == "chain":
        row_state, row_skip = R.case_graph(S)
        return (row_state,) + chain_as_lattice(row_skip) + (S,)
    if kind == "dense":
        pred = np.zeros((S, SLOTS), dtype=np.int32)
        for r in range(1, S):
            pred[r] = rng.randint(1, min(r, 300) + 1, SLOTS)
        flags = np.zeros(S, dtype=np.int32)
        n = min(4, S)
        flags[np.concatenate([[0], 1 + rng.choice(max(S // 2 - 1, n - 1), n - 1, replace=False)])] |= START
        flags[np.concatenate([[S - 1], S - 2 - rng.choice(max(S // 2 - 1, n - 1), n - 1, replace=False)])] |= FINAL
        return np.arange(S, dtype=np.int32), pred, flags, S
    K = 3 if S % 3 == 0 else (2 if S % 2 == 0 and S >= 16 else 1)
    units, P = S // K, 20
    boundary = units >= 3
    left, longest, words = units - (2 if boundary else 0), min(40, 1 + units // 8), []
    while left > 0:
        need = 1 if words else 0
        lens = [int(v) for v in rng.randint(1, longest + 1, rng.randint(1, 5))]
        if need + sum(lens) > left:
            if left - need < 1:  # one unit left and it would be the silence: the last word's last variant takes it
                words[-1][-1].append(int(rng.randint(P)))
                break
            lens = [left - need]
        words.append([[int(p) for p in rng.randint(P, size=n)] for n in lens])
        left -= need + sum(lens)
    g = word_graph(words, P, K, boundary)
    assert len(g["row_state"]) == S
    return g["row_state"], g["row_pred"], g["row_flags"], (P + 1) * K


@functools.lru_cache(maxsize=None)
def case_ll(M, T, seed):
    """float32 ll [T][M]: Gaussian noise around -30"""
    return (np.random.RandomState(seed).randn(T, M) * 2.0 - 30.0).astype(np.float32)


def path_score(ll, row_state, frame_row):
    return R.path_score(ll, row_state, frame_row)
