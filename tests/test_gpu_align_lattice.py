"""al_lattice_viterbi_kernel (csrc/align_lattice.hip) through the C ABI, Aligner.fit / align with lexicon= and `align --lexicon` against the numpy
statement of tests/align_lattice_ref.py.  The harness is test_gpu_align.py's: every buffer the kernel writes, the workspace included,
sits between guard zones of a NaN bit pattern that must survive, and every test reads the library's launch record and fails if its kernel did not
run.  The statement itself is checked against brute force in test_align_lattice_cpu.py."""
import functools
import json

import numpy as np
import pytest
import torch

import align_lattice_ref as L
import align_ref as R
import test_gpu_align as G
from test_gpu_align import speech  # noqa: F401  (the fixture: the tone-synthesised wavs of the chain driver's test)

pytestmark = pytest.mark.gpu
DEV = G.DEV
U = 2.0 ** -24
LATTICE, CHAIN = "al_lattice_viterbi_kernel", G.VITERBI
MCOL = G.MCOL


@pytest.fixture(scope="module")
def A():
    assert torch.cuda.is_available()
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib, alignment

    _lib.load()
    return alignment


def run_lattice(A, cases, workspace_bytes=None, n_states=MCOL, tamper=None):
    """ONE al_lattice_viterbi_kernel launch over cases [(ll float32 [T][n_states], row_state, row_pred, row_flags)] on guarded buffers ->
    test_gpu_align.guarded_launch's dicts; tamper(mp) may replace device tables first"""
    mp = A.AlignMaps([len(c[0]) for c in cases], [(c[1], np.asarray(c[2]).reshape(-1, 8), c[3]) for c in cases], n_states, DEV)
    assert mp.lattice
    pred, flags = G.Guarded(mp.rows * 8, torch.int32).set(mp.row_preds), G.Guarded(mp.rows, torch.int32).set(mp.row_flagss)
    mp.row_pred, mp.row_flags = pred.t, flags.t
    if tamper is not None:
        tamper(mp)

    def launch(*bufs):
        with G.launched(LATTICE, absent=(CHAIN,)):
            A.launch_lattice_viterbi(mp, *bufs)

    return G.guarded_launch(mp, cases, n_states, workspace_bytes, launch, tables=(pred, flags))


def case(size, kind):
    S, T = size
    row_state, pred, flags, M = L.case_lattice(S, kind)
    return G.padded(L.case_ll(M, T, 7 * S + T + len(kind))), row_state, pred, flags


@functools.lru_cache(maxsize=None)
def device_lattice(size, kind):
    """one single-utterance launch per case, shared by the tests that compare them"""
    from fcl_taco2_amd import alignment

    return run_lattice(alignment, [case(size, kind)])[0]


@functools.lru_cache(maxsize=None)
def reference(size, kind, dtype):
    ll, row_state, pred, flags = case(size, kind)
    return L.lattice_viterbi(ll, row_state, pred, flags, dtype=dtype)


def check_path(got, ll, row_state, pred, flags):
    """the path is valid for the lattice and row_begin / row_frames say what frame_row says"""
    S, T = len(row_state), len(ll)
    assert got["ok"] == 1 and L.path_valid(got["frame_row"], pred, flags) and (np.diff(got["frame_row"]) >= 0).all()
    begin, count = L.runs(got["frame_row"], S, got["frame0"])
    assert np.array_equal(got["row_frames"], count) and np.array_equal(got["row_begin"], begin) and count.sum() == T


def same(a, b):
    return (a["ok"] == b["ok"] and np.asarray(a["score"], np.float32).tobytes() == np.asarray(b["score"], np.float32).tobytes()
            and np.array_equal(a["frame_row"], b["frame_row"]) and np.array_equal(a["row_frames"], b["row_frames"])
            and np.array_equal(a["row_begin"] - a["frame0"], b["row_begin"] - b["frame0"]))


CASES = [(s, k) for s in L.SIZES for k in L.KINDS if L.fits(s[0], k)]


@pytest.mark.parametrize("size,kind", CASES, ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else v)
def test_lattice_vs_reference(A, size, kind):
    """The bounds of test_viterbi_vs_float64 (one rounded add per frame on either side): with gamma = 1.01 (T + 2) 2^-24 and A the sum of |ll| along the
    path, the path is valid for the lattice, the score is within gamma A of the float64 sum along the GPU's own path, and
    0 <= V64 - s64(G) <= 2.1 gamma A against the float64 optimum.  frame_row and score are the float32 statement's bit for bit."""
    S, T = size
    ll, row_state, pred, flags = case(size, kind)
    got, want = device_lattice(size, kind), reference(size, kind, np.float64)
    if not want["ok"]:
        assert kind != "dense" and size == (3, 2)  # three rows in a row and two frames
        G.check_failed(got, S, T)
        return
    check_path(got, ll, row_state, pred, flags)
    s64, absum = L.path_score(ll, row_state, got["frame_row"])
    gamma = 1.01 * (T + 2) * U
    assert abs(float(got["score"]) - s64) <= gamma * absum, (float(got["score"]), s64, gamma * absum)
    gap = float(want["score"]) - s64
    assert -T * 2.0 ** -52 * absum <= gap <= 2.1 * gamma * absum, (gap, gamma * absum)
    f32 = reference(size, kind, np.float32)
    assert np.array_equal(f32["frame_row"], got["frame_row"]) and np.float32(f32["score"]).tobytes() == got["score"].tobytes()


@pytest.mark.parametrize("kind", R.KINDS)
def test_a_chain_through_the_lattice_entry_is_the_chain_entry(A, kind):
    """every align_ref size through both entries, one launch each: frame_row, row_frames, score and ok bit for bit, row_begin on the rows with frames"""
    cases = [G.case(s, kind) for s in R.SIZES]
    chain = G.run_viterbi(A, cases)
    lattice = run_lattice(A, [(ll, rs) + L.chain_as_lattice(sk) for ll, rs, sk in cases])
    for s, c, g in zip(R.SIZES, chain, lattice):
        assert g["ok"] == c["ok"] == (s != (3, 2)) and g["score"].tobytes() == c["score"].tobytes() and np.array_equal(g["frame_row"], c["frame_row"]), s
        on = c["row_frames"] > 0
        assert np.array_equal(g["row_frames"], c["row_frames"]) and np.array_equal(g["row_begin"][on], c["row_begin"][on]), s
        assert (g["row_begin"][~on] == g["frame0"]).all()


def test_exact_chains_through_the_lattice_entry_bit_for_bit(A):
    """the exact-integer cases of the chain tests: both entries and the float64 statement agree bit for bit"""
    cases = [R.exact_case(K * (3 + seed % 5), 9 + 2 * seed + (seed % 3), K, 100 * K + seed) for K in (1, 2, 3) for seed in range(12)]
    M = max(c[0].shape[1] for c in cases)
    wide = [(np.pad(ll, ((0, 0), (0, M - ll.shape[1]))), rs, sk) for ll, rs, sk in cases]
    chain = G.run_viterbi(A, wide, n_states=M)
    lattice = run_lattice(A, [(ll, rs) + L.chain_as_lattice(sk) for ll, rs, sk in wide], n_states=M)
    n = 0
    for c, g, (ll, rs, sk) in zip(chain, lattice, cases):
        want = R.viterbi(ll, rs, sk)
        assert g["ok"] == c["ok"] == want["ok"] and g["score"].tobytes() == c["score"].tobytes() and np.array_equal(g["frame_row"], c["frame_row"])
        assert np.array_equal(g["row_frames"], c["row_frames"])
        if want["ok"]:
            assert np.array_equal(g["frame_row"], want["frame_row"]) and float(g["score"]) == float(want["score"])
            n += 1
    assert n >= 30


def test_long_predecessor_distances(A):
    """a dense case takes moves over more than 255 rows and a words case one over more than 100: a distance table stored too narrow fails here"""
    for size, kind, least in (((1024, 1024), "dense", 255), ((1024, 1024), "words", 100)):
        ll, row_state, pred, flags = case(size, kind)
        assert L.usable(pred).max() > least
        got = device_lattice(size, kind)
        f32 = reference(size, kind, np.float32)
        assert got["ok"] == 1 and np.array_equal(got["frame_row"], f32["frame_row"])  # truncated distances would offer other candidates to most rows
    # planted, so that the path itself takes such moves: the only way into the FINAL row is a move over 700 rows (slot 7), and one over 300 (slot 3) on the way
    S, T = 1024, 12
    pred, flags = np.zeros((S, 8), np.int32), np.zeros(S, np.int32)
    pred[1:, 0] = 1
    pred[S - 1] = [0, 0, 0, 0, 0, 0, 0, 700]
    pred[S - 1 - 700] = [0, 0, 0, 300, 0, 0, 0, 0]
    flags[S - 1 - 1000 - 3] |= L.START
    flags[S - 1] |= L.FINAL
    ll = G.padded(L.case_ll(S, T, 5))
    got = run_lattice(A, [(ll, np.arange(S, dtype=np.int32), pred, flags)])[0]
    want = L.lattice_viterbi(ll, np.arange(S), pred, flags, dtype=np.float32)
    assert want["ok"] == 1 and sorted(set(np.diff(want["frame_row"]))) == [0, 1, 300, 700]
    check_path(got, ll, np.arange(S), pred, flags)
    assert np.array_equal(got["frame_row"], want["frame_row"]) and got["score"].tobytes() == np.float32(want["score"]).tobytes()


def test_unreachable_end_fails_its_utterance_alone(A):
    """T below the shortest START -> FINAL path: ok 0 in the failure form; the neighbours in the batch are bit for bit their single launches"""
    row_state, pred, flags, M = L.case_lattice(257, "words")
    short = 3
    ll = G.padded(L.case_ll(M, short, 1))
    assert L.lattice_viterbi(ll, row_state, pred, flags)["ok"] == 0
    sizes = [((9, 9), "words"), ((255, 300), "dense")]
    got = run_lattice(A, [case(*sizes[0]), (ll, row_state, pred, flags), case(*sizes[1])])
    G.check_failed(got[1], 257, short)
    assert same(got[0], device_lattice(*sizes[0])) and same(got[2], device_lattice(*sizes[1])) and got[0]["ok"] == got[2]["ok"] == 1


def test_end_row_ties_go_to_the_lower_row(A):
    """integer-valued ll: FINAL rows far apart in the workgroup (rows of different threads and of one thread) tie on the score"""
    S, T = 600, 5
    pred, flags = np.zeros((S, 8), np.int32), np.zeros(S, np.int32)
    ends = [3, 40, 259, 515, 599]  # 3 and 259 and 515 are rows of one thread
    flags[ends] |= L.START | L.FINAL
    row_state = np.zeros(S, np.int32)
    row_state[ends] = [1, 2, 2, 1, 2]
    ll = np.full((T, MCOL), np.nan, np.float32)
    ll[:, :3] = [-50.0, -3.0, -2.0]
    for lose, win in (([], 40), ([40], 259), ([40, 259], 599)):  # the best rows are those of state 2: the lowest of them wins
        f = flags.copy()
        f[lose] = 0
        got = run_lattice(A, [(ll, row_state, pred, f)])[0]
        assert got["ok"] == 1 and (got["frame_row"] == win).all() and float(got["score"]) == -2.0 * T, (lose, got["frame_row"])
        want = L.lattice_viterbi(ll, row_state, pred, f, dtype=np.float32)
        assert np.array_equal(want["frame_row"], got["frame_row"])
        assert list(np.flatnonzero(got["row_frames"])) == [win] and (np.delete(got["row_begin"], win) == got["frame0"]).all()


def test_batch_is_bit_for_bit_its_single_launches(A):
    """every size and kind through ONE launch, interleaved (large beside small, the infeasible ones in the middle)"""
    order = [c for c in CASES[::2] + CASES[1::2] if c[0] != (1024, 4096)] + [((1024, 4096), "words")]
    got = run_lattice(A, [case(s, k) for s, k in order])
    for g, (s, k) in zip(got, order):
        assert same(g, device_lattice(s, k)), (s, k)


@pytest.mark.parametrize("size,kind", [((9, 9), "words"), ((257, 511), "dense")], ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else v)
def test_survives_non_finite_inputs(A, size, kind):
    """NaN and +-inf sprinkled over ll, a whole frame of NaN, of -inf, of +inf: ok 0 with the failed outputs, or a valid path; the guard zones are
    checked in run_lattice either way, and the finite neighbour in the same launch is untouched"""
    S, T = size
    ll, row_state, pred, flags = case(size, kind)
    M = L.case_lattice(S, kind)[3]
    rng = np.random.RandomState(S)
    variants = []
    for what in ("sprinkled", "nan frame", "-inf frame", "+inf frame"):
        bad = ll.copy()
        if what == "sprinkled":
            idx = rng.rand(T, M) < 0.05
            bad[:, :M][idx] = rng.choice([np.nan, np.inf, -np.inf], int(idx.sum())).astype(np.float32)
        else:
            bad[T // 2, :M] = {"nan frame": np.nan, "-inf frame": -np.inf, "+inf frame": np.inf}[what]
        variants.append(bad)
    rest = (row_state, pred, flags)
    got = run_lattice(A, [(v,) + rest for v in variants[:2]] + [(ll,) + rest] + [(v,) + rest for v in variants[2:]])
    clean = got.pop(2)
    assert clean["ok"] == 1 and same(clean, device_lattice(size, kind))
    for g, v in zip(got, variants):
        want = L.lattice_viterbi(v, row_state, pred, flags, dtype=np.float32)
        assert g["ok"] == want["ok"]
        if g["ok"]:
            check_path(g, ll, row_state, pred, flags)
            assert np.array_equal(g["frame_row"], want["frame_row"]) and np.isfinite(g["score"])
        else:
            G.check_failed(g, S, T)
    assert not got[1]["ok"] and not got[2]["ok"] and not got[3]["ok"]  # a whole frame that is not finite leaves no finite end


def test_fails_an_utterance_whose_slices_do_not_fit(A):
    """device tables the host cannot check: a cell slice one cell short, offsets far outside the buffers, a frame slice longer than max_t says --
    that utterance gets the failed outputs inside its clamped slices, the guard zones survive, the other one is bit for bit its single launch"""
    sizes = [((9, 9), "words"), ((257, 511), "dense")]
    cases = [case(*s) for s in sizes]
    one = device_lattice(*sizes[1])

    def short_cells(mp):
        off = mp.cell_offs.copy()
        off[1] -= 1
        mp.cell_off = torch.from_numpy(off).to(DEV)

    def wild_offsets(mp):
        mp.frame_off = torch.tensor([-5, 9, 1 << 30], dtype=torch.int32, device=DEV)
        mp.cell_off = torch.tensor([-(1 << 40), 81, 1 << 40], dtype=torch.int64, device=DEV)

    for tamper in (short_cells, wild_offsets):
        got = run_lattice(A, cases, tamper=tamper)
        if tamper is short_cells:
            G.check_failed(got[0], 9, 9)
        else:
            check_path(got[0], *cases[0])
        assert same(got[1], one) and got[1]["ok"] == 1

    def long_frames(mp):
        mp.max_t = 300

    got = run_lattice(A, cases, tamper=long_frames)
    check_path(got[0], *cases[0])
    G.check_failed(got[1], 257, 511)


def test_refusals_launch_nothing(A):
    from fcl_taco2_amd import _lib

    z = lambda n, dt=torch.float32: torch.zeros(n, device=DEV, dtype=dt)
    graph = lambda S: (np.zeros(S, np.int32), np.zeros((S, 8), np.int32), np.ones(S, np.int32) * 3)
    with G.launched(absent=(LATTICE, CHAIN)):
        for T, S, ws_bytes, code in ((4097, 3, None, "-2"), (10, 1025, None, "-2"), (10, 3, 0, "-5")):
            mp = A.AlignMaps([T], [graph(S)], 4, DEV)
            ws = z(mp.workspace_bytes() if ws_bytes is None else 16, torch.uint8)
            with pytest.raises(_lib.FclError, match="error %s" % code):
                A.launch_lattice_viterbi(mp, z(T * 4), ws, z(T, torch.int32), z(S, torch.int32), z(S, torch.int32), z(1), z(1, torch.int32))
        mp = A.AlignMaps([3], [graph(2)], 4, DEV)
        mp.n_utt = 0  # an empty batch is no error and no launch
        A.launch_lattice_viterbi(mp, z(12), z(256, torch.uint8), z(3, torch.int32), z(2, torch.int32), z(2, torch.int32), z(1), z(1, torch.int32))


def test_garbage_in_the_graph_tables_stays_inside_the_slices(A):
    """row_pred with negative values, values past r and huge ones, row_flags with bits above 1 and negative words, states outside the model: the
    guard zones survive (run_lattice) and the result is what the statement makes of the same tables, which ignores all of it"""
    rng = np.random.RandomState(3)
    cases = []
    for size, kind in (((9, 9), "words"), ((257, 511), "dense"), ((256, 256), "chain")):
        ll, row_state, pred, flags = case(size, kind)
        S = size[0]
        bad = pred.astype(np.int64)  # wrapped into int32 below
        hit = rng.rand(S, 8) < 0.3
        bad[hit] = rng.choice([-1, -(1 << 31), (1 << 31) - 1, 1 << 16, (1 << 16) + 1, 1024, 5000], int(hit.sum())) + (np.arange(S)[:, None] * (rng.rand(S, 8) < 0.5))[hit]
        bad_flags = flags | (rng.randint(0, 1 << 20, S).astype(np.int32) << 2)
        bad_flags[rng.rand(S) < 0.1] |= np.int32(-(1 << 31))
        cases.append((ll, row_state, bad.astype(np.int32), bad_flags.astype(np.int32)))
    got = run_lattice(A, cases)
    for g, (ll, row_state, pred, flags) in zip(got, cases):
        want = L.lattice_viterbi(ll, row_state, pred, flags, dtype=np.float32)
        assert g["ok"] == want["ok"]
        if g["ok"]:
            check_path(g, ll, row_state, pred, flags)
            assert np.array_equal(g["frame_row"], want["frame_row"]) and g["score"].tobytes() == np.float32(want["score"]).tobytes()
        else:
            G.check_failed(g, len(row_state), len(ll))
    assert sum(g["ok"] for g in got) >= 1
    # states outside the model are clamped into it: nothing is read outside ll
    ll, row_state, pred, flags = case((9, 9), "words")
    wild = row_state.copy()
    wild[::2] = [-7, 1 << 30, -(1 << 31), 5000, 1024][: len(wild[::2])]
    got = run_lattice(A, [(ll, row_state, pred, flags)], n_states=MCOL, tamper=lambda mp: setattr(mp, "row_state", torch.from_numpy(wild).to(DEV)))[0]
    want = L.lattice_viterbi(ll, np.clip(wild, 0, MCOL - 1), pred, flags, dtype=np.float32)
    assert got["ok"] == want["ok"] and (not got["ok"] or np.array_equal(got["frame_row"], want["frame_row"]))


# ---- fit ----------------------------------------------------------------------------------------------------------------------------------------------------
NAMES = ["p%d" % i for i in range(L.N_PHONES)] + ["sil"]


def word_inputs(c):
    """the corpus as the package takes it: a Lexicon over w0 .. w19, word transcripts, device features"""
    from fcl_taco2_amd import lexicon as X

    lex = X.Lexicon({"w%d" % w: [[NAMES[p] for p in v] for v in variants] for w, variants in enumerate(c["vocab"])})
    return lex, [["w%d" % w for w in words] for words, _ in c["picks"]], [torch.from_numpy(x) for x in c["feats"]]


@functools.lru_cache(maxsize=None)
def float64_trainer(seed):
    c = L.corpus(seed)
    mean, var, _ = L.fit(c["feats"], c["graphs"], c["M"], 4)
    counts, _ = L.align(c["feats"], c["graphs"], mean, var)
    return R.frame_accuracy(counts, c["codes"], c["truth"]), L.variant_accuracy(counts, c["graphs"], c["picks"], c["vocab"])[0]


@pytest.mark.parametrize("mixtures", [1, 2])
def test_fit_with_a_lexicon_reaches_the_float64_trainers_accuracy(A, mixtures):
    """Aligner.fit(lexicon=) on the word corpus, 4 rounds after the flat start, in two batches: the frame accuracy is at least the float64 trainer's
    less 0.002 (a float32 tie may move a boundary) and the share of multi-variant words given the variant of the recording at least its share less
    0.01 (variants that tie in float32 are as rare; one word in a hundred).  With mixtures = 2 the same lattice launch feeds the mixture entries.
    durations sum to T; the silences dropped are exactly those without frames; pronunciations are the variants of the rows on the path."""
    c = L.corpus(1)
    K = c["K"]
    lex, transcripts, feats = word_inputs(c)
    cells = sum(len(x) * len(g["row_state"]) for x, g in zip(c["feats"], c["graphs"]))
    al = A.Aligner(DEV, NAMES, K, optional=("sil",), batch_cells=cells // 2 + 1)
    extra = ("al_gmm_loglik_kernel", "al_gmm_post_kernel", "al_gmm_stats_kernel") if mixtures > 1 else ()
    with G.launched(G.LOGLIK, LATTICE, G.STATS, *extra, absent=(CHAIN,)):
        hist = al.fit(feats, transcripts, iterations=4, lexicon=lex, mixtures=mixtures, mix_iterations=2)
        res = al.align(feats, transcripts, lexicon=lex)
    rounds = 4 + (2 if mixtures > 1 else 0)
    assert len(hist["score"]) == rounds and hist["failed"] == [[]] * rounds and hist["score"][-1] > hist["score"][0]
    counts = [r["row_frames"] for r in res]
    for r, g in zip(res, c["graphs"]):  # the package's graph is the statement's
        assert np.array_equal(r["graph"].row_pred, g["row_pred"]) and np.array_equal(r["graph"].row_state, g["row_state"])
    acc = R.frame_accuracy(counts, c["codes"], c["truth"])
    var_acc, n_multi = L.variant_accuracy(counts, c["graphs"], c["picks"], c["vocab"])
    ref_acc, ref_var = float64_trainer(1)
    print("fit with a lexicon, mixtures %d: frame accuracy %.4f on the device, %.4f in float64; variants right %.4f of %d on the device, %.4f in float64"
          % (mixtures, acc, ref_acc, var_acc, n_multi, ref_var))
    assert ref_acc >= 0.98 and ref_var >= 0.95 and n_multi >= 80
    assert acc >= ref_acc - 0.002 and var_acc >= ref_var - 0.01
    for r, g, x, tr in zip(res, c["graphs"], c["feats"], transcripts):
        per = r["row_frames"].reshape(-1, K).sum(axis=1)
        word, variant, phone = g["row_word"][::K], g["row_variant"][::K], g["row_phone"][::K]
        on = per > 0
        assert r["ok"] and sum(r["durations"]) == len(x) and r["durations"] == [int(n) for n in per[on]] and r["words"] == tr
        assert r["phones"] == [NAMES[p] for p in phone[on]] and r["label_words"] == [int(w) for w in word[on]]
        assert (word[~on & (phone == L.SIL)] == -1).all() and r["phones"].count("sil") == int((on & (word < 0)).sum())  # dropped silences: those with 0 frames
        assert r["pronunciations"] == list(L.chosen_variants(g, r["row_frames"])) and min(r["pronunciations"]) >= 0
        assert r["word_durations"] == [int(per[word == i].sum()) for i in range(len(tr))] and min(r["word_durations"]) >= K
        assert sum(r["word_durations"]) + sum(d for d, w in zip(r["durations"], r["label_words"]) if w < 0) == len(x)
    if mixtures > 1:
        assert al.model.is_mixture and hist["components"][-1] > hist["components"][0]


# ---- driver -------------------------------------------------------------------------------------------------------------------------------------------------
WORD_OF = dict(aa="ah", iy="ee", uw="oo", sh="shh")
LEXICON = "# tones\nAH aa\nEE iy\nOO uw\nSHH sh\nWILD aa\nWILD(2) iy\n"


def word_transcripts(speech):  # noqa: F811
    """the recordings in words: every tone is its own word, but a last tone `aa` or `iy` is written WILD, whose two pronunciations are those two
    tones (every recording also holds both of them under their own words) -> (lines, {aligned utt: the variant the recording holds})"""
    lines, held = [], {}
    for u in speech["ids"]:
        words = [WORD_OF[p].capitalize() for p in speech["transcripts"][u] if p != "sp"]
        last = speech["transcripts"][u][-1]
        if last in ("aa", "iy"):
            words[-1] = "Wild,"
            if u in speech["truth"]:
                held[u] = ("aa", "iy").index(last)
        lines.append(u + " " + " ".join(words))
    return lines, held


def test_driver_aligns_words_through_a_lexicon(A, speech, tmp_path):  # noqa: F811
    """python -m fcl_taco2_amd.align --lexicon on the tone recordings: both tiers, `phones` read back by read_textgrid + alignment to the durations
    written; the words tier spans the phones; --pronunciations-out names the tones that were synthesised; that file as --transcripts of the chain
    driver with --model gives the same phones"""
    from fcl_taco2_amd import align as drv, textgrid as TG

    root = speech["root"]
    lines, held = word_transcripts(speech)
    (tmp_path / "words.txt").write_text("\n".join(lines) + "\n")
    (tmp_path / "lex.txt").write_text(LEXICON)
    common = ["--wav-dir", str(root / "wavs"), "--verbose", "0"]
    with G.launched("fx_logmel_kernel<1024>", "ev_cepstra_kernel", G.LOGLIK, LATTICE, G.STATS, absent=(CHAIN,)):
        doc = drv.main(common + ["--transcripts", str(tmp_path / "words.txt"), "--lexicon", str(tmp_path / "lex.txt"), "--optional", "sp", "--textgrid-out",
                                 str(tmp_path / "tg"), "--durations-out", str(tmp_path / "dur"), "--model-out", str(tmp_path / "m.npz"), "--iterations", "6",
                                 "--pronunciations-out", str(tmp_path / "pron.txt"), "--report", str(tmp_path / "rep.json")])
    assert json.load(open(tmp_path / "rep.json")) == doc and doc["n_utt"] == 9 and doc["not_aligned"] == ["crowded"]
    assert doc["settings"]["phones"] == sorted(list(G.TONES) + ["sp"]) and doc["lexicon"]["skipped"] == {} and doc["lexicon"]["boundary_silence"] is True
    n_aa = sum(1 for v in held.values() if v == 0)
    assert doc["lexicon"]["variants"]["wild"] == [n_aa, len(held) - n_aa] and 0 < n_aa < len(held) and set(doc["lexicon"]["variants"]) == {"ah", "ee", "oo", "shh", "wild"}
    prons = dict((ln.split()[0], ln.split()[1:]) for ln in open(tmp_path / "pron.txt"))
    assert sorted(prons) == sorted(u for u in speech["ids"] if u != "crowded")
    for u, phones in prons.items():
        labels, frames, n_samples = speech["truth"][u]
        T = n_samples // G.HOP + 1
        assert [p for p in phones if p != "sp"] == [p for p in labels if p != "sp"]  # WILD as the tone that was synthesised
        dur = [int(d) for d in np.load(tmp_path / "dur" / (u + ".npy"))]
        assert sum(dur) == T and len(dur) == len(phones) and min(dur) >= 1
        tiers = TG.read_textgrid(str(tmp_path / "tg" / (u + ".TextGrid")))
        assert list(tiers) == ["phones", "words"]
        got_phones, got = TG.alignment(tiers["phones"], G.FS, G.HOP)
        assert got_phones == phones[:-1] + ["sil" if phones[-1] == "sp" else phones[-1]] and got == dur[:-1] + [dur[-1] - 1]
        assert [t for _, _, t in tiers["phones"]] == phones
        # the words tier: the words in order, silences as empty text, every word from its first phone's start to its last phone's end
        words = [w.strip(",").lower() for w in dict((ln.split()[0], ln.split()[1:]) for ln in lines)[u]]
        assert [t for _, _, t in tiers["words"] if t] == words
        edges = {a for a, _, _ in tiers["phones"]} | {tiers["phones"][-1][1]}
        assert tiers["words"][0][0] == 0 and tiers["words"][-1][1] == tiers["phones"][-1][1] and all(a in edges and b in edges for a, b, _ in tiers["words"])
        assert all(a[1] == b[0] for a, b in zip(tiers["words"], tiers["words"][1:]))
        spans = [(a, b) for a, b, t in tiers["phones"] if t == "sp"]
        assert [(a, b) for a, b, t in tiers["words"] if not t] == spans  # one tone per word here: the silences of both tiers coincide
    # the chosen pronunciations as phoneme transcripts of the chain driver, with the model just trained
    with G.launched(G.LOGLIK, CHAIN, absent=(LATTICE, G.STATS)):
        doc2 = drv.main(common + ["--transcripts", str(tmp_path / "pron.txt"), "--model", str(tmp_path / "m.npz"), "--textgrid-out", str(tmp_path / "tg2")])
    assert doc2["n_utt"] == doc2["n_aligned"] == 8 and "lexicon" not in doc2
    for u, phones in prons.items():
        tiers = TG.read_textgrid(str(tmp_path / "tg2" / (u + ".TextGrid")))
        assert list(tiers) == ["phones"] and [t for _, _, t in tiers["phones"]] == phones


def test_driver_out_of_lexicon_words(A, speech, tmp_path):  # noqa: F811
    """--oov refuse lists the words with their counts before any device call; --oov skip leaves the utterances out and names them in the report"""
    from fcl_taco2_amd import align as drv

    root = speech["root"]
    lines, _ = word_transcripts(speech)
    lines = [ln for ln in lines if not ln.startswith("crowded")]
    lines[1] += " Zebra zebra!"
    lines[4] += " gnu"
    (tmp_path / "words.txt").write_text("\n".join(lines) + "\n")
    (tmp_path / "lex.txt").write_text(LEXICON)
    base = ["--wav-dir", str(root / "wavs"), "--verbose", "0", "--transcripts", str(tmp_path / "words.txt"), "--lexicon", str(tmp_path / "lex.txt"), "--optional", "sp",
            "--textgrid-out", str(tmp_path / "tg")]
    with G.launched(absent=(G.LOGLIK, LATTICE, CHAIN, G.STATS, "fx_logmel_kernel<1024>")):
        with pytest.raises(ValueError, match=r"2 words .* \(in 2 utterances.*\): gnu \(1\), zebra \(2\)$"):
            drv.main(base)
        with pytest.raises(SystemExit):
            drv.main(base + ["--optional", "sp", "sil"])  # the silence must be one label
        (tmp_path / "lex2.txt").write_text(LEXICON + "ZEBRA zz iy\nGNU aa\n")
        with pytest.raises(ValueError, match="label 'zz' is not in the inventory"):
            A.AlignModel(sorted(list(G.TONES) + ["sp"]), 3, np.zeros((15, 28)), np.ones((15, 28))).save(str(tmp_path / "m.npz"))
            drv.main(base[:6] + ["--lexicon", str(tmp_path / "lex2.txt"), "--optional", "sp", "--textgrid-out", str(tmp_path / "tg"), "--model", str(tmp_path / "m.npz")])
    ids = [ln.split()[0] for ln in lines]
    with G.launched(LATTICE, absent=(CHAIN,)):
        doc = drv.main(base + ["--oov", "skip", "--iterations", "2", "--no-boundary-silence"])
    assert doc["lexicon"]["skipped"] == {ids[1]: ["zebra"], ids[4]: ["gnu"]} and doc["n_utt"] == 6 == doc["n_aligned"] and doc["lexicon"]["boundary_silence"] is False
    assert sorted(p.name for p in (tmp_path / "tg").iterdir()) == sorted(u + ".TextGrid" for k, u in enumerate(ids) if k not in (1, 4))
