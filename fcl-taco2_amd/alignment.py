"""Forced alignment on the HIP path: flat-start Viterbi training of monophone models -- single Gaussians, optionally grown into mixtures of up to 8
diagonal Gaussians per state -- and the alignment they give (csrc/align.hip, csrc/align_gmm.hip).

What Kaldi's monophone pass and HTK's flat start do: start from an equal segmentation of every utterance over its transcript, then alternate a
Viterbi alignment with a re-estimation of the Gaussians, and keep the last alignment.  Every phoneme of the inventory has K left-to-right states
without transition probabilities; a phoneme named optional (a pause between words) may be skipped as a whole.  The E-step runs on the device
(log-likelihoods, Viterbi with its backtrack, statistics in float64), the M-step on the host in float64.  The contract is stated in
include/fcl_hip.h "Forced alignment" and restated in float64 numpy in tests/align_ref.py (the mixture entries: tests/align_gmm_ref.py).  Agreement with the Montreal Forced Aligner on real
recordings stays unpinned: neither that tool nor real speech is available here.

    al = Aligner("cuda:0", phones, states=3, optional=("sp",))
    history = al.fit(features, transcripts, iterations=15)      # features: per utterance [T, D] on the device; mixtures=4 grows mixtures
    results = al.align(features, transcripts)                   # per utterance: phones, durations in frames (summing to T), score

With lexicon= (lexicon.Lexicon) the transcripts are words: every word contributes all its pronunciations side by side, the one optional label stands
as a silence between the words and at both ends, and the Viterbi over that lattice picks pronunciations and pauses (csrc/align_lattice.hip, DESIGN.md
§6x; restated in tests/align_lattice_ref.py).  Everything around the Viterbi launch is shared with the chain path.

No CPU fallback."""
import collections
import ctypes as C
import math

import numpy as np
import torch

from . import _lib, lexicon as LX, metrics, ops

STATES_DEFAULT, STATES_MAX, MODEL_STATES_MAX, DIM_MAX, FRAMES_MAX, ROWS_MAX, UTT_MAX = 3, 3, 1024, 40, 4096, 1024, 65535
BATCH_CELLS = 16 << 20
BATCH_LL = 1 << 28  # frames x M of one batch's log-likelihood matrix (the entries need it below 2^31)
VAR_FLOOR = 0.01
ORDER, DELTA_WINDOW, ENERGY_FLOOR = 13, 2, 1e-10
ITERATIONS_DEFAULT = 15  # not tuned: the synthetic corpora of the tests converge within 6
MIXTURES_MAX, COMPONENTS_MAX, MIX_ITERATIONS_DEFAULT, MIN_OCCUPANCY_DEFAULT = 8, 8192, 4, 10.0
WEIGHT_FLOOR, SPLIT = 1e-5, 0.2
PRED_SLOTS, START, FINAL = 8, 1, 2  # fcl_al_lattice_t: predecessor slots per row, the bits of row_flags


# ---- model ------------------------------------------------------------------------------------------------------------------------------------------
def gconst(var):
    """gconst[m] = -0.5 (D ln 2pi + sum_d ln var[m][d]), float64"""
    var = np.asarray(var, dtype=np.float64)
    return -0.5 * (var.shape[1] * math.log(2.0 * math.pi) + np.log(var).sum(axis=1))


class AlignModel(object):
    """phones (the inventory, in index order), K states per phoneme, mean / var [M = len(phones) K][D] in float64, and the settings of the
    features they were trained on (a dict of plain values; a model is only good for features made the same way).  With the keywords weight [G] and
    comp_off [M + 1] the states are mixtures: state m owns the components comp_off[m] .. comp_off[m + 1] (1 .. 8 of them, G <= 8192 in all) of
    mean / var [G][D], and their weights sum to 1 inside a state.  Without them every state has one component of weight 1."""

    def __init__(self, phones, states, mean, var, settings=None, weight=None, comp_off=None):
        self.phones, self.K = [str(p) for p in phones], int(states)
        check_inventory(self.phones, self.K)
        self.mean, self.var = np.array(mean, dtype=np.float64), np.array(var, dtype=np.float64)
        self.settings = dict(settings or {})
        M = len(self.phones) * self.K
        if (weight is None) != (comp_off is None):
            raise ValueError("fcl-taco2_amd: alignment: a mixture model needs both weight and comp_off")
        if comp_off is None:
            if self.mean.ndim != 2 or self.mean.shape != self.var.shape or self.mean.shape[0] != M or not 1 <= self.mean.shape[1] <= DIM_MAX:
                raise ValueError("fcl-taco2_amd: alignment: mean / var must be [%d states][1 .. %d], got %r and %r" % (M, DIM_MAX, self.mean.shape, self.var.shape))
            self.weight, self.comp_off = np.ones(M), np.arange(M + 1, dtype=np.int32)
        else:
            self.weight, self.comp_off = np.array(weight, dtype=np.float64).reshape(-1), np.array(comp_off, dtype=np.int64).reshape(-1)
            counts = np.diff(self.comp_off)
            if len(self.comp_off) != M + 1 or self.comp_off[0] != 0 or counts.min() < 1 or counts.max() > MIXTURES_MAX or self.comp_off[-1] > COMPONENTS_MAX:
                raise ValueError("fcl-taco2_amd: alignment: comp_off must give each of the %d states 1 .. %d components, at most %d in all" % (M, MIXTURES_MAX, COMPONENTS_MAX))
            G = int(self.comp_off[-1])
            self.comp_off = self.comp_off.astype(np.int32)
            if self.mean.ndim != 2 or self.mean.shape != self.var.shape or self.mean.shape[0] != G or not 1 <= self.mean.shape[1] <= DIM_MAX or len(self.weight) != G:
                raise ValueError("fcl-taco2_amd: alignment: mean / var must be [%d components][1 .. %d] and weight [%d], got %r, %r and %r"
                                 % (G, DIM_MAX, G, self.mean.shape, self.var.shape, self.weight.shape))
            if not (np.isfinite(self.weight).all() and (self.weight > 0).all()):
                raise ValueError("fcl-taco2_amd: alignment: the model needs positive finite component weights")
        if not (np.isfinite(self.mean).all() and np.isfinite(self.var).all() and (self.var > 0).all()):
            raise ValueError("fcl-taco2_amd: alignment: the model needs finite means and positive finite variances")

    @property
    def n_states(self):
        return len(self.comp_off) - 1

    @property
    def n_components(self):
        return self.mean.shape[0]

    @property
    def max_components(self):
        return int(np.diff(self.comp_off).max())

    @property
    def is_mixture(self):
        """any state with more than one component"""
        return self.n_components > self.n_states

    @property
    def dim(self):
        return self.mean.shape[1]

    def params32(self):
        """(mean, ivar, gconst) as uploaded: formed in float64, rounded to float32"""
        return self.mean.astype(np.float32), (1.0 / self.var).astype(np.float32), gconst(self.var).astype(np.float32)

    def gmm_params32(self):
        """(mean [G][D], ivar [G][D], cconst [G] = ln w + gconst(var), comp_off [M + 1] int32) as uploaded to the mixture entries"""
        return (self.mean.astype(np.float32), (1.0 / self.var).astype(np.float32), (np.log(self.weight) + gconst(self.var)).astype(np.float32),
                self.comp_off.astype(np.int32))

    def upload(self, dev):
        """the device tensors of params32(), or of gmm_params32() for a mixture model"""
        return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (self.gmm_params32() if self.is_mixture else self.params32()))

    def save(self, path):
        import json

        extra = dict(weight=self.weight, comp_off=self.comp_off.astype(np.int32)) if self.is_mixture else {}  # a one-component model writes today's file
        with open(path, "wb") as f:
            np.savez(f, phones=np.asarray(self.phones), states=np.int64(self.K), mean=self.mean, var=self.var,
                     settings=np.asarray(json.dumps(self.settings, sort_keys=True)), **extra)

    @classmethod
    def load(cls, path):
        import json

        with np.load(path, allow_pickle=False) as z:
            missing = [k for k in ("phones", "states", "mean", "var", "settings") if k not in z.files]
            if missing:
                raise ValueError("%s: not an alignment model (no %s)" % (path, ", ".join(missing)))
            mix = dict(weight=z["weight"], comp_off=z["comp_off"]) if "comp_off" in z.files and "weight" in z.files else {}
            return cls([str(p) for p in z["phones"]], int(z["states"]), z["mean"], z["var"], json.loads(str(z["settings"])), **mix)


def check_inventory(phones, states):
    if not 1 <= int(states) <= STATES_MAX:
        raise ValueError("fcl-taco2_amd: alignment: --states %r must lie in 1 .. %d" % (states, STATES_MAX))
    if len(set(phones)) != len(phones) or not phones:
        raise ValueError("fcl-taco2_amd: alignment: the phoneme inventory must be non-empty and without duplicates")
    if len(phones) * int(states) > MODEL_STATES_MAX:
        raise ValueError("fcl-taco2_amd: alignment: %d phonemes x %d states exceed %d model states" % (len(phones), int(states), MODEL_STATES_MAX))


# ---- utterance graph --------------------------------------------------------------------------------------------------------------------------------
def build_graph(labels, index, optional, K, utt="#?"):
    """A transcript -> (row_state, row_skip, row_phone) int32: K rows per phoneme, row_skip[a + K] = K + 1 behind an optional phoneme on the rows
    [a, a + K).  Refused naming the utterance: a label that is not in the inventory, an optional phoneme that is first, last or next to another
    optional one, no labels, more than 1024 rows."""
    labels = list(labels)
    if not labels:
        raise ValueError("fcl-taco2_amd: alignment: utterance %s has an empty transcript" % utt)
    for p in labels:
        if p not in index:
            raise ValueError("fcl-taco2_amd: alignment: utterance %s: label %r is not in the inventory" % (utt, p))
    n = len(labels)
    if n * K > ROWS_MAX:
        raise ValueError("fcl-taco2_amd: alignment: utterance %s has %d phonemes x %d states = %d rows; the alignment covers at most %d"
                         % (utt, n, K, n * K, ROWS_MAX))
    opt = [p in optional for p in labels]
    row_skip = np.zeros(n * K, dtype=np.int32)
    for i in np.flatnonzero(opt):
        if i == 0 or i == n - 1:
            raise ValueError("fcl-taco2_amd: alignment: utterance %s: the optional phoneme %r is the %s label; an optional phoneme needs a mandatory "
                             "one on either side" % (utt, labels[i], "first" if i == 0 else "last"))
        if opt[i - 1] or opt[i + 1]:
            raise ValueError("fcl-taco2_amd: alignment: utterance %s: the optional phonemes %r and %r are next to each other (labels %d and %d)"
                             % (utt, labels[i - 1 if opt[i - 1] else i], labels[i if opt[i - 1] else i + 1], i - 1 if opt[i - 1] else i,
                                i if opt[i - 1] else i + 1))
        row_skip[(i + 1) * K] = K + 1
    row_state = np.asarray([index[p] * K + k for p in labels for k in range(K)], dtype=np.int32)
    return row_state, row_skip, np.repeat(np.arange(n, dtype=np.int32), K)


def optional_rows(row_skip):
    """the rows a skip jumps over"""
    opt = np.zeros(len(row_skip), dtype=bool)
    for r in np.flatnonzero(np.asarray(row_skip) >= 2):
        opt[r - int(row_skip[r]) + 1 : r] = True
    return opt


def uniform_alignment(T, row_skip):
    """row_frames [S] int64 of the equal split of T frames: over all rows when T >= S, over the mandatory rows otherwise; None when the mandatory
    rows alone do not fit.  Row i of the n rows taken gets floor((i + 1) T / n) - floor(i T / n) frames."""
    S = len(row_skip)
    rows = np.arange(S) if T >= S else np.flatnonzero(~optional_rows(row_skip))
    n = len(rows)
    if n == 0 or T < n:
        return None
    out = np.zeros(S, dtype=np.int64)
    out[rows] = np.diff((np.arange(n + 1, dtype=np.int64) * int(T)) // n)
    return out


WordGraph = collections.namedtuple("WordGraph", "row_state row_pred row_flags row_phone row_word row_variant")


def build_word_graph(words, lex, index, silence, K, boundary=True, utt="#?"):
    """A word transcript -> WordGraph(row_state, row_pred [S][8], row_flags, row_phone, row_word, row_variant), int32: the lattice
    [sil_0] w_0 [sil_1] w_1 ... w_(n-1) [sil_n].  Every word is the concatenation of its pronunciations' chains (K rows per label), every silence K rows
    of the label `silence`; sil_0 and sil_n exist only with `boundary`.  Predecessor slots: 1 on slot 0 of an inner row; on the first row of sil_i
    (i >= 1) the last rows of the variants of w_(i-1) in variant order; on the first row of a variant of w_i the last row of sil_i first, where there
    is one, then the last rows of the variants of w_(i-1) in variant order.  START: the first rows of sil_0 and of the variants of w_0; FINAL: the last
    rows of sil_n and of the variants of w_(n-1).  row_phone is the inventory index of the row's label, row_word / row_variant the word and the
    variant of a word row and -1 on a silence row.  The tokens are normalised (lexicon.normalise), those of which nothing is left are dropped.
    Refused naming the utterance: no words, words the lexicon lacks (all of them named), a label that is not in the inventory, more than 1024 rows."""
    words = LX.normalise_words(words)
    if not words:
        raise ValueError("fcl-taco2_amd: alignment: utterance %s has an empty transcript" % utt)
    missing = sorted(set(w for w in words if lex.lookup(w) is None))
    if missing:
        raise ValueError("fcl-taco2_amd: alignment: utterance %s: not in the lexicon: %s" % (utt, ", ".join(missing)))
    prons = [lex.lookup(w)[: LX.VARIANTS_MAX] for w in words]
    for p in [silence] + [p for vs in prons for v in vs for p in v]:
        if p not in index:
            raise ValueError("fcl-taco2_amd: alignment: utterance %s: label %r is not in the inventory" % (utt, p))
    n = len(words)
    S = K * (sum(len(v) for vs in prons for v in vs) + n - 1 + (2 if boundary else 0))
    if S > ROWS_MAX:
        raise ValueError("fcl-taco2_amd: alignment: utterance %s: %d words with their pronunciations and silences make %d rows; the alignment covers at most %d"
                         % (utt, n, S, ROWS_MAX))
    row_state, row_phone, row_word, row_variant = (np.zeros(S, dtype=np.int32) for _ in range(4))
    row_pred, row_flags = np.zeros((S, PRED_SLOTS), dtype=np.int32), np.zeros(S, dtype=np.int32)
    r = 0

    def chain(labels, word, variant):
        """lays the rows of `labels` from r on -> (first row, last row)"""
        nonlocal r
        first = r
        for p in labels:
            for k in range(K):
                row_state[r], row_phone[r], row_word[r], row_variant[r] = index[p] * K + k, index[p], word, variant
                if r > first:
                    row_pred[r, 0] = 1
                r += 1
        return first, r - 1

    def enter(row, sources):
        for slot, src in enumerate(sources):
            row_pred[row, slot] = row - src

    ends = []  # the last rows of the previous word's variants
    for i in range(n + 1):
        sil = None
        if boundary or 0 < i < n:
            sil = chain([silence], -1, -1)
            enter(sil[0], ends)
            if i == 0:
                row_flags[sil[0]] |= START
            if i == n:
                row_flags[sil[1]] |= FINAL
        if i == n:
            break
        new_ends = []
        for v, labels in enumerate(prons[i]):
            first, last = chain(labels, i, v)
            enter(first, ([sil[1]] if sil else []) + ends)
            if i == 0:
                row_flags[first] |= START
            if i == n - 1:
                row_flags[last] |= FINAL
            new_ends.append(last)
        ends = new_ends
    assert r == S
    return WordGraph(row_state, row_pred, row_flags, row_phone, row_word, row_variant)


def canonical_rows(graph, boundary=True):
    """the rows of the canonical chain of a WordGraph: the first-listed variant of every word, with sil_0 and sil_n (the silence rows before the first
    and behind the last word row) when `boundary`"""
    word = np.flatnonzero(graph.row_word >= 0)
    keep = graph.row_variant == 0
    if boundary:
        r = np.arange(len(graph.row_word))
        keep = keep | ((graph.row_word < 0) & ((r < word[0]) | (r > word[-1])))
    return np.flatnonzero(keep)


def uniform_word_alignment(T, graph):
    """row_frames [S] int64 of the flat start of a WordGraph: the equal split of uniform_alignment over the canonical chain -- sil_0, the first-listed
    variant of every word, sil_n --, without the two silences when T is below that row count, None when that does not fit either.  Inter-word
    silences and the other variants get no frames."""
    for boundary in (True, False):
        rows = canonical_rows(graph, boundary)
        n = len(rows)
        if n and T >= n:
            out = np.zeros(len(graph.row_state), dtype=np.int64)
            out[rows] = np.diff((np.arange(n + 1, dtype=np.int64) * int(T)) // n)
            return out
    return None


def flat_start(T, graph):
    """the flat-start row_frames of a chain (row_state, row_skip, ...) or of a WordGraph"""
    return uniform_word_alignment(T, graph) if isinstance(graph, WordGraph) else uniform_alignment(T, graph[1])


def mstep(n, s, q, mean, var, var_floor=VAR_FLOOR):
    """float64 on the host: mean = s / n, var = max(q / n - mean^2, var_floor x global variance); a state with n < 2 keeps its parameters"""
    n, s, q = np.asarray(n, dtype=np.float64), np.asarray(s, dtype=np.float64), np.asarray(q, dtype=np.float64)
    N = n.sum()
    if N < 2:
        raise _lib.FclError("fcl-taco2_amd: alignment: no aligned frames to estimate the model from")
    gmean = s.sum(axis=0) / N
    floor = float(var_floor) * (q.sum(axis=0) / N - gmean * gmean)
    mean, var = np.array(mean, dtype=np.float64), np.array(var, dtype=np.float64)
    for m in np.flatnonzero(n >= 2):
        mean[m] = s[m] / n[m]
        var[m] = np.maximum(q[m] / n[m] - mean[m] * mean[m], floor)
    return mean, var


def global_model(n, s, q, n_states):
    """every state at the global mean and variance of the frames counted: the parameters a state keeps that the flat start gives fewer than 2 frames"""
    N = float(np.sum(n))
    gmean = np.sum(s, axis=0) / N
    return np.tile(gmean, (n_states, 1)), np.tile(np.sum(q, axis=0) / N - gmean * gmean, (n_states, 1))


def mixture_targets(mixtures):
    """the component targets of the mixture stage: 2, 4, ... and the last one is `mixtures` itself (none for 1)"""
    out, t = [], 2
    while t < mixtures:
        out.append(t)
        t *= 2
    return out + ([int(mixtures)] if mixtures > 1 else [])


def split_components(mean, var, weight, occ, comp_off, target, min_occupancy=MIN_OCCUPANCY_DEFAULT):
    """Per state, while it has fewer than `target` components: the component of largest weight (the first on ties) is split unless its occupancy is
    below 2 min_occupancy, which ends the splitting of this state.  A split halves weight and occupancy; the component moves to mean + 0.2 sigma and
    a copy at mean - 0.2 sigma with the same variance is appended at the end of the state's list.  float64 on the host.
    -> (mean, var, weight, occ, comp_off) of the grown model"""
    mean, var, weight, occ = (np.asarray(v, dtype=np.float64) for v in (mean, var, weight, occ))
    out_m, out_v, out_w, out_o, off = [], [], [], [], [0]
    for m in range(len(comp_off) - 1):
        a, b = int(comp_off[m]), int(comp_off[m + 1])
        mu, va, w, o = [r.copy() for r in mean[a:b]], [r.copy() for r in var[a:b]], [float(v) for v in weight[a:b]], [float(v) for v in occ[a:b]]
        while len(w) < target:
            j = int(np.argmax(w))
            if o[j] < 2.0 * min_occupancy:
                break
            w[j], o[j] = w[j] / 2.0, o[j] / 2.0
            step = SPLIT * np.sqrt(va[j])
            mu.append(mu[j] - step)
            va.append(va[j].copy())
            w.append(w[j])
            o.append(o[j])
            mu[j] = mu[j] + step
        out_m, out_v, out_w, out_o = out_m + mu, out_v + va, out_w + w, out_o + o
        off.append(len(out_w))
    return np.asarray(out_m), np.asarray(out_v), np.asarray(out_w), np.asarray(out_o), np.asarray(off, dtype=np.int32)


def mstep_mixtures(w, s, q, mean, var, weight, comp_off, var_floor=VAR_FLOOR):
    """float64 on the host: a component with w >= 2 gets mean = s / w and var = max(q / w - mean^2, var_floor x global variance of this pass), the
    others keep their parameters; a state whose occupancy (the sum of its w) is >= 2 gets the weights max(w / occupancy, 1e-5), renormalised"""
    w, s, q = np.asarray(w, dtype=np.float64), np.asarray(s, dtype=np.float64), np.asarray(q, dtype=np.float64)
    N = w.sum()
    if N < 2:
        raise _lib.FclError("fcl-taco2_amd: alignment: no aligned frames to estimate the model from")
    gmean = s.sum(axis=0) / N
    floor = float(var_floor) * (q.sum(axis=0) / N - gmean * gmean)
    mean, var, weight = np.array(mean, dtype=np.float64), np.array(var, dtype=np.float64), np.array(weight, dtype=np.float64)
    for g in np.flatnonzero(w >= 2):
        mean[g] = s[g] / w[g]
        var[g] = np.maximum(q[g] / w[g] - mean[g] * mean[g], floor)
    for m in range(len(comp_off) - 1):
        a, b = int(comp_off[m]), int(comp_off[m + 1])
        occ = w[a:b].sum()
        if occ >= 2:
            v = np.maximum(w[a:b] / occ, WEIGHT_FLOOR)
            weight[a:b] = v / v.sum()
    return mean, var, weight


# ---- packed batches -----------------------------------------------------------------------------------------------------------------------------------
class AlignMaps(object):
    """The tables of a packed batch on the device: frame_off / row_off [n + 1] int32, cell_off [n + 1] int64 (cumulative S T), row_state /
    row_skip [rows] int32, and the batch's rows grouped by model state (state_off [M + 1], state_rows [rows]: ascending row index inside a group),
    with their totals on the host.  Graphs whose second table has two dimensions are lattices (WordGraph, or (row_state, row_pred [S][8],
    row_flags)): the maps then carry row_pred [rows][8] / row_flags [rows] for fcl_al_lattice_viterbi_fwd and `lattice` is True."""

    def __init__(self, frame_lens, graphs, n_states, dev):
        self.frame_lens = [int(t) for t in frame_lens]
        self.row_lens = [len(g[0]) for g in graphs]
        assert len(self.frame_lens) == len(self.row_lens)
        self.n_utt, self.n_states = len(self.frame_lens), int(n_states)
        cum = lambda v: np.concatenate([[0], np.cumsum(np.asarray(v, dtype=np.int64))]).astype(np.int64)
        self.frame_offs, self.row_offs = cum(self.frame_lens), cum(self.row_lens)
        self.cell_offs = cum([t * s for t, s in zip(self.frame_lens, self.row_lens)])
        self.frames, self.rows, self.cells = int(self.frame_offs[-1]), int(self.row_offs[-1]), int(self.cell_offs[-1])
        self.max_t, self.max_s = max(self.frame_lens + [0]), max(self.row_lens + [0])
        self.row_states = np.concatenate([np.asarray(g[0], dtype=np.int32) for g in graphs]) if graphs else np.zeros(0, np.int32)
        self.lattice = bool(graphs) and np.ndim(graphs[0][1]) == 2
        if self.lattice:
            assert all(np.ndim(g[1]) == 2 and np.shape(g[1])[1] == PRED_SLOTS for g in graphs)
            self.row_preds = np.concatenate([np.asarray(g[1], dtype=np.int32) for g in graphs])
            self.row_flagss = np.concatenate([np.asarray(g[2], dtype=np.int32) for g in graphs])
            graphs = [(g[0], np.zeros(len(g[0]), np.int32)) for g in graphs]  # no row_skip: the chain entry is not for these maps
        self.row_skips = np.concatenate([np.asarray(g[1], dtype=np.int32) for g in graphs]) if graphs else np.zeros(0, np.int32)
        self.max_skip = int(self.row_skips.max()) if self.rows else 0
        self.state_rows_h = np.argsort(self.row_states, kind="stable").astype(np.int32)
        self.state_offs = cum(np.bincount(self.row_states, minlength=self.n_states))
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
        self.frame_off, self.row_off, self.cell_off = t(self.frame_offs, np.int32), t(self.row_offs, np.int32), t(self.cell_offs, np.int64)
        self.row_state, self.row_skip = t(self.row_states, np.int32), t(self.row_skips, np.int32)
        self.state_off, self.state_rows = t(self.state_offs, np.int32), t(self.state_rows_h, np.int32)
        if self.lattice:
            self.row_pred, self.row_flags = t(self.row_preds, np.int32), t(self.row_flagss, np.int32)

    @property
    def frame_utt(self):
        """[frames] int64 on the device: the utterance of each frame (built on first use: only the mixture stage needs it)"""
        if getattr(self, "_frame_utt", None) is None:
            self._frame_utt = torch.from_numpy(np.repeat(np.arange(self.n_utt, dtype=np.int64), self.frame_lens)).to(self.frame_off.device)
        return self._frame_utt

    def workspace_bytes(self):
        return int(_lib.load().fcl_al_workspace_bytes(self.cells, self.n_utt))


# one launch each, on caller-owned buffers (the tests surround them with guard zones)
def launch_loglik(params, x, ll, frames):
    """params: (mean [M][D], ivar [M][D], gconst [M]) float32 on the device; x [frames][D] -> ll [frames][M]"""
    mean, ivar, gc = params
    _lib.check(_lib.load().fcl_al_loglik_fwd(x.data_ptr(), mean.data_ptr(), ivar.data_ptr(), gc.data_ptr(), ll.data_ptr(), int(frames), int(mean.shape[1]),
                                             int(mean.shape[0]), ops._stream()))


def _viterbi_args(a, mp, ll, workspace, frame_row, row_begin, row_frames, score, ok):
    """the fields Align and AlignLattice share: the batch's sizes and tables, ll, the workspace and the outputs -> a"""
    a.frames, a.rows, a.cells = mp.frames, mp.rows, mp.cells
    a.n_utt, a.n_states, a.max_t, a.max_s = mp.n_utt, mp.n_states, mp.max_t, mp.max_s
    a.frame_off, a.row_off, a.cell_off, a.row_state = mp.frame_off.data_ptr(), mp.row_off.data_ptr(), mp.cell_off.data_ptr(), mp.row_state.data_ptr()
    a.ll, a.workspace, a.workspace_bytes = ll.data_ptr(), workspace.data_ptr(), int(workspace.numel() * workspace.element_size())
    a.frame_row, a.row_begin, a.row_frames, a.score, a.ok = (v.data_ptr() for v in (frame_row, row_begin, row_frames, score, ok))
    return a


def launch_viterbi(mp, ll, workspace, frame_row, row_begin, row_frames, score, ok):
    """ll [frames][M] float32 -> frame_row [frames], row_begin / row_frames [rows], ok [n_utt] int32, score [n_utt] float32; workspace: uint8,
    AlignMaps.workspace_bytes() of it"""
    a = _viterbi_args(_lib.Align(), mp, ll, workspace, frame_row, row_begin, row_frames, score, ok)
    a.max_skip, a.row_skip = mp.max_skip, mp.row_skip.data_ptr()
    _lib.check(_lib.load().fcl_al_viterbi_fwd(C.byref(a), ops._stream()))


def launch_lattice_viterbi(mp, ll, workspace, frame_row, row_begin, row_frames, score, ok):
    """launch_viterbi over the lattices of mp (AlignMaps.lattice): fcl_al_lattice_viterbi_fwd on mp.row_pred / mp.row_flags"""
    a = _viterbi_args(_lib.AlignLattice(), mp, ll, workspace, frame_row, row_begin, row_frames, score, ok)
    a.row_pred, a.row_flags = mp.row_pred.data_ptr(), mp.row_flags.data_ptr()
    _lib.check(_lib.load().fcl_al_lattice_viterbi_fwd(C.byref(a), ops._stream()))


def launch_stats(mp, x, row_begin, row_frames, acc_n, acc_s, acc_q):
    """x [frames][D] float32 over the rows' runs: ADDS to acc_n [M] int64, acc_s / acc_q [M][D] float64"""
    _lib.check(_lib.load().fcl_al_stats_fwd(x.data_ptr(), row_begin.data_ptr(), row_frames.data_ptr(), mp.state_off.data_ptr(), mp.state_rows.data_ptr(),
                                            acc_n.data_ptr(), acc_s.data_ptr(), acc_q.data_ptr(), mp.frames, mp.rows, int(acc_s.shape[1]), mp.n_states,
                                            ops._stream()))


def launch_gmm_loglik(params, x, ll, frames, max_comp=MIXTURES_MAX):
    """params: (mean [G][D], ivar [G][D], cconst [G] float32, comp_off [M + 1] int32) on the device; x [frames][D] -> ll [frames][M]; max_comp: the
    largest component count of a state (the kernels read no more of any state)"""
    mean, ivar, cc, comp_off = params
    _lib.check(_lib.load().fcl_al_gmm_loglik_fwd(x.data_ptr(), mean.data_ptr(), ivar.data_ptr(), cc.data_ptr(), comp_off.data_ptr(), ll.data_ptr(), int(frames),
                                                 int(mean.shape[1]), int(comp_off.numel()) - 1, int(mean.shape[0]), int(max_comp), ops._stream()))


def launch_gmm_post(params, x, frame_state, gamma, frames, max_comp=MIXTURES_MAX):
    """frame_state [frames] int32 (the model state the alignment gave each frame, -1: none) -> gamma [frames][8] float32"""
    mean, ivar, cc, comp_off = params
    _lib.check(_lib.load().fcl_al_gmm_post_fwd(x.data_ptr(), mean.data_ptr(), ivar.data_ptr(), cc.data_ptr(), comp_off.data_ptr(), frame_state.data_ptr(),
                                               gamma.data_ptr(), int(frames), int(mean.shape[1]), int(comp_off.numel()) - 1, int(mean.shape[0]), int(max_comp),
                                               ops._stream()))


def launch_gmm_stats(mp, comp_off, x, gamma, row_begin, row_frames, acc_w, acc_s, acc_q, max_comp=MIXTURES_MAX):
    """x [frames][D] and gamma [frames][8] float32 over the rows' runs: ADDS to acc_w [G], acc_s / acc_q [G][D] float64"""
    _lib.check(_lib.load().fcl_al_gmm_stats_fwd(x.data_ptr(), gamma.data_ptr(), row_begin.data_ptr(), row_frames.data_ptr(), mp.state_off.data_ptr(),
                                                mp.state_rows.data_ptr(), comp_off.data_ptr(), acc_w.data_ptr(), acc_s.data_ptr(), acc_q.data_ptr(), mp.frames,
                                                mp.rows, int(acc_s.shape[1]), mp.n_states, int(acc_s.shape[0]), int(max_comp), ops._stream()))


def frame_states(mp, frame_row):
    """frame_state [frames] int32 on the device, by torch indexing: the model state of the row the alignment gave each frame, -1 for the frames of
    an utterance without an alignment (frame_row -1)"""
    row = mp.row_off.long()[mp.frame_utt] + frame_row.long()
    return torch.where(frame_row >= 0, mp.row_state[row.clamp(min=0, max=max(mp.rows - 1, 0))], torch.full_like(frame_row, -1)).to(torch.int32).contiguous()


def utt_batches(frame_lens, row_lens, batch_cells, n_states=1):
    """consecutive runs of utterances whose cells S T sum to at most batch_cells (a larger single utterance goes alone) and whose frames x M stay
    below BATCH_LL, at most 65535 utterances each"""
    out, cur, cells, frames = [], [], 0, 0
    for i, (t, s) in enumerate(zip(frame_lens, row_lens)):
        c = int(t) * int(s)
        if cur and (cells + c > batch_cells or (frames + int(t)) * n_states > BATCH_LL or len(cur) >= UTT_MAX):
            out.append(cur)
            cur, cells, frames = [], 0, 0
        cur.append(i)
        cells, frames = cells + c, frames + int(t)
    return out + ([cur] if cur else [])


# ---- features -----------------------------------------------------------------------------------------------------------------------------------------
def deltas(x, window=DELTA_WINDOW):
    """[T, C] -> the regression deltas over +-window frames with replicated edges: sum_n n (x[t + n] - x[t - n]) / (2 sum_n n^2)"""
    T = x.shape[0]
    idx = torch.arange(T, device=x.device)
    out = torch.zeros_like(x)
    for n in range(1, window + 1):
        out = out + float(n) * (x[torch.clamp(idx + n, max=T - 1)] - x[torch.clamp(idx - n, min=0)])
    return out / (2.0 * sum(n * n for n in range(1, window + 1)))


def feature_settings(plan, order=ORDER):
    """the settings an AlignModel carries: the analysis of the FeaturePlan and the make of the features"""
    return dict(fs=plan.fs, n_fft=plan.n_fft, hop=plan.hop, win_length=plan.win_length, n_mels=plan.A, fmin=plan.fmin, fmax=plan.fmax, order=int(order),
                delta_window=DELTA_WINDOW, dim=2 * (int(order) + 1))


class AlignFeatures(object):
    """FeatureExtractor output -> the aligner's features, torch expressions on the device: `order` cepstra of the raw log-mel (metrics.CepstraPlan)
    with the utterance mean subtracted, the log frame energy minus its utterance maximum, and the deltas of both over +-2 frames with replicated
    edges: D = 2 (order + 1) = 28."""

    def __init__(self, extractor, order=ORDER):
        if extractor.plan.mel_stats is not None:
            raise ValueError("fcl-taco2_amd: alignment: the feature extractor must give raw log10 mels (no mel_stats)")
        self.extractor, self.order = extractor, int(order)
        self.cepstra = metrics.CepstraPlan(extractor.plan.device, extractor.plan.A, self.order)
        self.dim = 2 * (self.order + 1)
        self.settings = feature_settings(extractor.plan, self.order)

    def from_mel(self, mel, energy, frame_lens):
        """mel [sum T, n_mels] raw log10, energy [sum T] -> list of [T, D] float32 device tensors"""
        dev = self.extractor.plan.device
        with torch.cuda.device(dev):
            c = torch.empty(mel.shape[0], self.order, device=dev, dtype=torch.float32)
            metrics.launch_cepstra(self.cepstra, mel.contiguous(), c, mel.shape[0])
            le = torch.log(torch.clamp(energy.to(torch.float32), min=ENERGY_FLOOR))
            out, o = [], 0
            for T in frame_lens:
                cu, eu = c[o : o + T], le[o : o + T]
                base = torch.cat([cu - cu.mean(dim=0, keepdim=True), (eu - eu.max()).unsqueeze(1)], dim=1)
                out.append(torch.cat([base, deltas(base)], dim=1).contiguous())
                o += T
        return out

    def from_waves(self, waves, ids=None):
        """list of 1-D float waveforms at the analysis rate -> list of [T, D] device tensors: one mel launch, one cepstra launch"""
        xs = [np.asarray(w, dtype=np.float32).reshape(-1) for w in waves]
        mel, energy, frame_lens = self.extractor.extract_packed(np.concatenate(xs), [len(x) for x in xs], ids=ids)
        return self.from_mel(mel, energy, frame_lens)


def check_features(features, ids=None):
    """per-utterance [T, D] tensors -> (frame counts, D); another shape, more than one D, D > 40 and T outside 1 .. 4096 are refused by id"""
    D = None
    for i, x in enumerate(features):
        name = ids[i] if ids is not None else "#%d" % i
        if x.dim() != 2 or not 1 <= x.shape[1] <= DIM_MAX or (D is not None and x.shape[1] != D):
            raise ValueError("fcl-taco2_amd: alignment: utterance %s: features %r; [T, D] with one 1 <= D <= %d expected" % (name, tuple(x.shape), DIM_MAX))
        D = int(x.shape[1])
        if not 1 <= x.shape[0] <= FRAMES_MAX:
            raise ValueError("fcl-taco2_amd: alignment: utterance %s has %d frames; the alignment covers 1 .. %d" % (name, x.shape[0], FRAMES_MAX))
    return [int(x.shape[0]) for x in features], D


# ---- the aligner --------------------------------------------------------------------------------------------------------------------------------------
class _RoundTally(object):
    """one round of Aligner.fit: the score total and the frames of the utterances with an alignment, the names of those without"""

    def __init__(self, frame_lens, name):
        self.frame_lens, self.name, self.total, self.frames, self.failed = frame_lens, name, 0.0, 0, []

    def batch(self, idx, ok, score):
        """a batch's ok / score device tensors, idx: its utterances"""
        okh, sh = ok.cpu().numpy(), score.cpu().numpy().astype(np.float64)
        for k, i in enumerate(idx):
            if okh[k]:
                self.total, self.frames = self.total + sh[k], self.frames + self.frame_lens[i]
            else:
                self.failed.append(self.name(i))

    def close(self, history, components):
        """the round's entries of fit's history"""
        history["score"].append(self.total / max(self.frames, 1))
        history["failed"].append(self.failed)
        history["components"].append(components)


class Aligner(object):
    """Flat-start training and alignment.  phones: the inventory; optional: the labels that may be skipped (pauses); model: an AlignModel to align
    with (fit replaces it); settings: what the model is to carry about its features."""

    def __init__(self, device, phones=None, states=STATES_DEFAULT, optional=(), model=None, var_floor=VAR_FLOOR, batch_cells=BATCH_CELLS, settings=None):
        if not str(device).startswith("cuda"):
            raise _lib.FclError("fcl-taco2_amd: Aligner needs a GPU device (no CPU fallback)")
        if model is not None:
            phones, states = model.phones, model.K
        check_inventory(list(phones or []), states)
        if batch_cells < 1:
            raise ValueError("fcl-taco2_amd: alignment: --batch-cells must be positive (got %r)" % (batch_cells,))
        self.device, self.phones, self.K = torch.device(device), [str(p) for p in phones], int(states)
        self.index = {p: i for i, p in enumerate(self.phones)}
        self.optional = set(str(p) for p in optional)
        for p in sorted(self.optional):
            if p not in self.index:
                raise ValueError("fcl-taco2_amd: alignment: the optional label %r is not in the inventory" % p)
        self.n_states = len(self.phones) * self.K
        self.model, self.var_floor, self.batch_cells, self.settings = model, float(var_floor), int(batch_cells), dict(settings or {})

    # -- preparation: everything that can be refused is refused before the first launch
    def _prepare(self, features, transcripts, ids, lex=None, boundary=True):
        if len(features) != len(transcripts):
            raise _lib.FclError("fcl-taco2_amd: alignment: %d feature matrices for %d transcripts" % (len(features), len(transcripts)))
        features[:] = [torch.as_tensor(x) for x in features]
        name = lambda i: ids[i] if ids is not None else "#%d" % i
        if lex is not None:
            graphs = [build_word_graph(tr, lex, self.index, self.silence(), self.K, boundary, name(i)) for i, tr in enumerate(transcripts)]
        else:
            graphs = [build_graph(tr, self.index, self.optional, self.K, name(i)) for i, tr in enumerate(transcripts)]
        return (graphs,) + check_features(features, ids)

    def silence(self):
        """the silence label of the word lattices: with a lexicon `optional` must name exactly one label"""
        if len(self.optional) != 1:
            raise ValueError("fcl-taco2_amd: alignment: with a lexicon `optional` names exactly one label, the silence (got %s)"
                             % (", ".join(sorted(self.optional)) or "none"))
        return next(iter(self.optional))

    def _batches(self, features, graphs, frame_lens):
        """[(indices, AlignMaps, x [frames][D])] of the consecutive batches"""
        dev = self.device
        for idx in utt_batches(frame_lens, [len(g[0]) for g in graphs], self.batch_cells, self.n_states):
            mp = AlignMaps([frame_lens[i] for i in idx], [graphs[i] for i in idx], self.n_states, dev)
            x = torch.cat([torch.as_tensor(features[i]).to(device=dev, dtype=torch.float32) for i in idx]).contiguous()
            yield idx, mp, x

    def _viterbi(self, mp, x, params):
        """one batch: log-likelihoods and Viterbi -> (row_begin, row_frames, score, ok) device tensors"""
        return self._viterbi_rows(mp, x, params)[:4]

    def _viterbi_rows(self, mp, x, params, max_comp=MIXTURES_MAX):
        """_viterbi and frame_row; params of four (AlignModel.gmm_params32) take the mixture log-likelihood"""
        dev = self.device
        ll = torch.empty(mp.frames, mp.n_states, device=dev, dtype=torch.float32)
        if len(params) == 4:
            launch_gmm_loglik(params, x, ll, mp.frames, max_comp)
        else:
            launch_loglik(params, x, ll, mp.frames)
        ws = torch.empty(mp.workspace_bytes(), device=dev, dtype=torch.uint8)
        frame_row = torch.empty(mp.frames, device=dev, dtype=torch.int32)
        row_begin, row_frames = torch.empty(mp.rows, device=dev, dtype=torch.int32), torch.empty(mp.rows, device=dev, dtype=torch.int32)
        score, ok = torch.empty(mp.n_utt, device=dev, dtype=torch.float32), torch.empty(mp.n_utt, device=dev, dtype=torch.int32)
        (launch_lattice_viterbi if mp.lattice else launch_viterbi)(mp, ll, ws, frame_row, row_begin, row_frames, score, ok)
        return row_begin, row_frames, score, ok, frame_row

    def _acc(self, D):
        dev = self.device
        return (torch.zeros(self.n_states, device=dev, dtype=torch.int64), torch.zeros(self.n_states, D, device=dev, dtype=torch.float64),
                torch.zeros(self.n_states, D, device=dev, dtype=torch.float64))

    def fit(self, features, transcripts, iterations=ITERATIONS_DEFAULT, ids=None, callback=None, mixtures=1, mix_iterations=MIX_ITERATIONS_DEFAULT,
            min_occupancy=MIN_OCCUPANCY_DEFAULT, lexicon=None, boundary=True):
        """features: per utterance a [T, D] tensor; transcripts: per utterance its labels -- with lexicon= (lexicon.Lexicon) its words: the graphs are
        then the lattices of build_word_graph (boundary: a silence at both ends), the flat start that of uniform_word_alignment, and the Viterbi launch
        is fcl_al_lattice_viterbi_fwd; everything else is shared.  The flat start, then `iterations` times align and
        re-estimate.  With mixtures > 1 the component target per state then doubles -- 2, 4, ..., the last target is `mixtures` --; at each target
        the components are split (split_components) and `mix_iterations` rounds of Viterbi alignment and re-estimation follow, soft inside a state:
        the component posteriors of the frames the path gave to that state (csrc/align_gmm.hip), the M-step on the host (mstep_mixtures).
        -> dict(score: the mean score per aligned frame of each round, failed: per round the utterances without an alignment (ids, or positions),
        components: the component total of each round); self.model is the trained AlignModel.  callback(round, model) runs after every
        re-estimation."""
        if not 1 <= int(mixtures) <= MIXTURES_MAX or int(mix_iterations) < 0 or not float(min_occupancy) >= 1.0:
            raise ValueError("fcl-taco2_amd: alignment: mixtures must lie in 1 .. %d, mix_iterations must not be negative and min_occupancy must be at least 1 "
                             "(got %r, %r, %r)" % (MIXTURES_MAX, mixtures, mix_iterations, min_occupancy))
        features = list(features)
        graphs, frame_lens, D = self._prepare(features, transcripts, ids, lexicon, boundary)
        name = lambda i: ids[i] if ids is not None else i
        with torch.cuda.device(self.device):
            batches = list(self._batches(features, graphs, frame_lens))
            acc = self._acc(D)
            for idx, mp, x in batches:  # the flat start: the statistics of the equal split
                flat = [flat_start(frame_lens[i], graphs[i]) for i in idx]
                counts = np.concatenate([np.zeros(len(graphs[i][0]), np.int64) if c is None else c for i, c in zip(idx, flat)])
                begin = np.concatenate([mp.frame_offs[k] + np.concatenate([[0], np.cumsum(c)[:-1]]) if c is not None else np.zeros(len(graphs[i][0]), np.int64)
                                        for k, (i, c) in enumerate(zip(idx, flat))])
                t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(self.device)
                launch_stats(mp, x, t(begin), t(counts), *acc)
            n, s, q = (v.cpu().numpy() for v in acc)
            mean, var = mstep(n, s, q, *global_model(n, s, q, self.n_states), var_floor=self.var_floor)
            self.model = AlignModel(self.phones, self.K, mean, var, self.settings)
            history = dict(score=[], failed=[], components=[])
            for it in range(int(iterations)):
                params, acc = self.model.upload(self.device), self._acc(D)
                tally = _RoundTally(frame_lens, name)
                for idx, mp, x in batches:
                    row_begin, row_frames, score, ok = self._viterbi(mp, x, params)
                    launch_stats(mp, x, row_begin, row_frames, *acc)
                    tally.batch(idx, ok, score)
                n, s, q = (v.cpu().numpy() for v in acc)
                mean, var = mstep(n, s, q, self.model.mean, self.model.var, var_floor=self.var_floor)
                self.model = AlignModel(self.phones, self.K, mean, var, self.settings)
                tally.close(history, self.n_states)
                if callback is not None:
                    callback(it, self.model)
            # ---- the mixture stage: from one component of weight 1 per state, the occupancies those of the last round (or of the flat start)
            mean, var, weight = self.model.mean, self.model.var, np.ones(self.n_states)
            occ, comp_off, it = np.asarray(n, dtype=np.float64), np.arange(self.n_states + 1, dtype=np.int32), int(iterations)
            for target in mixture_targets(mixtures):
                mean, var, weight, occ, comp_off = split_components(mean, var, weight, occ, comp_off, target, min_occupancy)
                self.model = AlignModel(self.phones, self.K, mean, var, self.settings, weight=weight, comp_off=comp_off)
                for _ in range(int(mix_iterations)):
                    G, max_comp = self.model.n_components, self.model.max_components
                    params = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(self.device) for a in self.model.gmm_params32())
                    acc = (torch.zeros(G, device=self.device, dtype=torch.float64), torch.zeros(G, D, device=self.device, dtype=torch.float64),
                           torch.zeros(G, D, device=self.device, dtype=torch.float64))
                    tally = _RoundTally(frame_lens, name)
                    for idx, mp, x in batches:
                        row_begin, row_frames, score, ok, frame_row = self._viterbi_rows(mp, x, params, max_comp)
                        gamma = torch.empty(mp.frames, MIXTURES_MAX, device=self.device, dtype=torch.float32)
                        launch_gmm_post(params, x, frame_states(mp, frame_row), gamma, mp.frames, max_comp)
                        launch_gmm_stats(mp, params[3], x, gamma, row_begin, row_frames, *acc, max_comp=max_comp)
                        tally.batch(idx, ok, score)
                    w, s, q = (v.cpu().numpy() for v in acc)
                    mean, var, weight = mstep_mixtures(w, s, q, mean, var, weight, comp_off, var_floor=self.var_floor)
                    occ = w
                    self.model = AlignModel(self.phones, self.K, mean, var, self.settings, weight=weight, comp_off=comp_off)
                    tally.close(history, G)
                    if callback is not None:
                        callback(it, self.model)
                    it += 1
        return history

    def align(self, features, transcripts, ids=None, lexicon=None, boundary=True):
        """-> per utterance dict(ok, score, phones, durations, row_frames): durations in frames on the features' grid, summing to T, the skipped
        optional phonemes dropped from phones and durations; an utterance without an alignment has ok False and phones / durations None.
        With lexicon= the transcripts are words and the entries also hold words (normalised), pronunciations (the chosen variant's index per word),
        word_durations (frames per word), label_words (per entry of phones its word, -1 for a silence) and graph (the WordGraph); phones / durations
        run along the chosen path, the silences that received frames included and the others dropped."""
        if self.model is None:
            raise _lib.FclError("fcl-taco2_amd: alignment: no model (fit first, or pass model=)")
        features = list(features)
        graphs, frame_lens, D = self._prepare(features, transcripts, ids, lexicon, boundary)
        if D is not None and D != self.model.dim:
            raise ValueError("fcl-taco2_amd: alignment: the features have %d coefficients, the model %d" % (D, self.model.dim))
        out = [None] * len(features)
        with torch.cuda.device(self.device):
            params, max_comp = self.model.upload(self.device), self.model.max_components  # a model with mixtures takes the mixture entries
            for idx, mp, x in self._batches(features, graphs, frame_lens):
                _, row_frames, score, ok, _ = self._viterbi_rows(mp, x, params, max_comp)
                rf, okh, sh = row_frames.cpu().numpy().astype(np.int64), ok.cpu().numpy(), score.cpu().numpy()
                for k, i in enumerate(idx):
                    c = rf[mp.row_offs[k] : mp.row_offs[k + 1]]
                    if not okh[k]:
                        out[i] = dict(ok=False, score=float("-inf"), phones=None, durations=None, row_frames=c)
                        if lexicon is not None:
                            out[i].update(words=LX.normalise_words(transcripts[i]), pronunciations=None, word_durations=None, label_words=None, graph=graphs[i])
                        continue
                    if lexicon is not None:
                        out[i] = dict(ok=True, score=float(sh[k]), row_frames=c, **self._word_result(transcripts[i], graphs[i], c))
                        continue
                    per = c.reshape(-1, self.K).sum(axis=1)
                    keep = [j for j, p in enumerate(transcripts[i]) if per[j] > 0 or p not in self.optional]
                    out[i] = dict(ok=True, score=float(sh[k]), phones=[transcripts[i][j] for j in keep], durations=[int(per[j]) for j in keep], row_frames=c)
        return out

    def _word_result(self, words, graph, row_frames):
        """words, pronunciations, word_durations, phones, durations and label_words of the path row_frames marks through a WordGraph"""
        K, words = self.K, LX.normalise_words(words)
        per = row_frames.reshape(-1, K).sum(axis=1)  # frames per label of the lattice
        word, variant, phone = graph.row_word[::K], graph.row_variant[::K], graph.row_phone[::K]
        on = np.flatnonzero(per > 0)
        pron, wdur = [-1] * len(words), [0] * len(words)
        for j in on:
            if word[j] >= 0:
                pron[word[j]], wdur[word[j]] = int(variant[j]), wdur[word[j]] + int(per[j])
        return dict(words=words, pronunciations=pron, word_durations=wdur, phones=[self.phones[phone[j]] for j in on], durations=[int(per[j]) for j in on],
                    label_words=[int(word[j]) for j in on], graph=graph)
