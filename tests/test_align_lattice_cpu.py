"""The numpy statement of the lattice Viterbi (tests/align_lattice_ref.py) against brute force and against the chain statement, the pronunciation
lexicon, the word graphs of alignment.build_word_graph, their flat start and refusals, the new C entry's validation, and the float64 trainer on the
synthetic word corpus.  No GPU; the kernel itself is compared with the statement in test_gpu_align_lattice.py."""
import ctypes as C
import logging
import os
import subprocess

import numpy as np
import pytest

import align_lattice_ref as L
import align_ref as R
from conftest import ROOT


@pytest.fixture(scope="module")
def A():
    from fcl_taco2_amd import alignment

    return alignment


# ---- the statement --------------------------------------------------------------------------------------------------------------------------------------
def test_the_statement_equals_brute_force_ties_included():
    """every seeded lattice with S <= 6 and T <= 6, integer-valued ll: the path, the score and ok of the recurrence are those of the enumeration
    of all valid paths under the global form of the tie rules; in float32 too (integers are exact)"""
    solved = tied = failed = 0
    for seed in range(400):
        ll, row_state, pred, flags = L.tiny_lattice(seed)
        want = L.brute_force(ll, row_state, pred, flags)
        for dtype in (np.float64, np.float32):
            got = L.lattice_viterbi(ll, row_state, pred, flags, dtype=dtype)
            assert got["ok"] == want["ok"], seed
            if not want["ok"]:
                assert got["score"] == -np.inf and (got["frame_row"] == -1).all() and not got["row_frames"].any()
                continue
            assert float(got["score"]) == want["score"] and np.array_equal(got["frame_row"], want["frame_row"]), (seed, got["frame_row"], want["frame_row"])
            assert L.path_valid(got["frame_row"], pred, flags) and got["row_frames"].sum() == len(ll)
        solved, tied, failed = solved + want["ok"], tied + (want["ok"] and want["n_tied"] > 1), failed + (not want["ok"])
    assert solved >= 200 and tied >= 100 and failed >= 20, (solved, tied, failed)


def test_paths_written_by_hand():
    ll = np.zeros((3, 2))
    pred, flags = np.zeros((2, 8), np.int32), np.asarray([L.START | L.FINAL, L.START | L.FINAL], np.int32)
    got = L.lattice_viterbi(ll, [0, 1], pred, flags)  # two rows that tie: the lower end row
    assert got["ok"] == 1 and list(got["frame_row"]) == [0, 0, 0] and list(got["row_frames"]) == [3, 0] and list(got["row_begin"]) == [0, 0]
    ll[:, 1] = 1.0
    got = L.lattice_viterbi(ll, [0, 1], pred, flags, frame0=7)
    assert list(got["frame_row"]) == [1, 1, 1] and got["score"] == 3.0 and list(got["row_begin"]) == [7, 7]
    pred[1] = [5, 0, -3, 1, 1, 0, 0, 0]  # slot 0 points before row 0 and does not count: the move from row 0 is slot 3's
    got = L.lattice_viterbi(np.asarray([[1.0, 0.0], [0.0, 1.0]]), [0, 1], pred, [L.START, L.FINAL])
    assert list(got["frame_row"]) == [0, 1] and L.path_valid([0, 1], pred, [L.START, L.FINAL]) and not L.path_valid([0, 1], pred * 0, [L.START, L.FINAL])
    assert L.lattice_viterbi(np.zeros((1, 2)), [0, 1], pred, [L.START, L.FINAL])["ok"] == 0  # one frame cannot hold START and FINAL on two rows
    assert L.lattice_viterbi(np.zeros((2, 2)), [0, 1], pred, [L.START | 4, 8])["ok"] == 0  # the flag bits above 1 say nothing


@pytest.mark.parametrize("kind", R.KINDS)
def test_a_chain_written_as_a_lattice_is_the_chain(kind):
    """align_ref.SIZES up to 257 rows and the exact-integer cases: frame_row, row_frames, score and ok of align_ref.viterbi, in both precisions, and
    row_begin on the rows with frames"""
    cases = [(R.case_ll(S, T, kind), *R.case_graph(S)) for S, T in R.SIZES if S <= 257]
    cases += [R.exact_case(K * (3 + seed % 5), 9 + 2 * seed + (seed % 3), K, 100 * K + seed) for K in (1, 2, 3) for seed in range(12)]
    failed = 0
    for ll, row_state, row_skip in cases:
        pred, flags = L.chain_as_lattice(row_skip)
        for dtype in (np.float64, np.float32):
            want, got = R.viterbi(ll, row_state, row_skip, dtype=dtype), L.lattice_viterbi(ll, row_state, pred, flags, dtype=dtype)
            assert got["ok"] == want["ok"] and np.array_equal(got["frame_row"], want["frame_row"]) and np.array_equal(got["row_frames"], want["row_frames"])
            assert np.asarray(got["score"], dtype=dtype).tobytes() == np.asarray(want["score"], dtype=dtype).tobytes()
            on = want["row_frames"] > 0
            assert np.array_equal(got["row_begin"][on], want["row_begin"][on])
            failed += not want["ok"]
    assert failed >= 2  # (3, 2) and the exact cases that do not fit are there


def test_case_lattices_are_what_they_say():
    for S in sorted(set(s for s, _ in L.SIZES)):
        for kind in L.KINDS:
            if not L.fits(S, kind):
                continue
            row_state, pred, flags, M = L.case_lattice(S, kind)
            assert len(row_state) == S == len(pred) == len(flags) and pred.shape[1] == 8 and 0 <= row_state.min() and row_state.max() < M <= 1024
            assert (flags & L.START).any() and (flags & L.FINAL).any()
            if kind == "dense":
                assert ((flags & L.START) > 0).sum() == 4 == ((flags & L.FINAL) > 0).sum() and (L.usable(pred)[1:] > 0).all()
    assert L.usable(L.case_lattice(1024, "dense")[1]).max() > 255 and L.usable(L.case_lattice(1024, "words")[1]).max() > 100


# ---- the lexicon ----------------------------------------------------------------------------------------------------------------------------------------
def test_lexicon_parser(tmp_path, caplog):
    from fcl_taco2_amd import lexicon as X

    many = "".join("MANY(%d) M %d\n" % (i + 1, i) for i in range(9))
    (tmp_path / "lex.txt").write_text(";;; a comment\n# another\n\nTHE DH AH0\nTHE(2) DH IY0\nthe(3)  DH   AH0\nDON'T D OW1 N T\nwell-known W EH1 L N OW1 N\n"
                                      "READ R EH1 D\nREAD(2) R IY1 D\n" + many)
    with caplog.at_level(logging.WARNING):
        lex = X.read_lexicon(str(tmp_path / "lex.txt"))
    assert lex.lookup("the") == [["DH", "AH0"], ["DH", "IY0"]]  # the suffix is stripped, the duplicate merged, file order kept
    assert lex.lookup("Read,") == [["R", "EH1", "D"], ["R", "IY1", "D"]] and lex.lookup('"Don\'t!"') == [["D", "OW1", "N", "T"]]
    assert lex.lookup("Well-Known") is not None and lex.lookup("well") is None and "the" in lex and "zebra" not in lex and len(lex) == 5
    assert lex.lookup("many") == [["M", str(i)] for i in range(7)] and lex.truncated == ["many"]
    assert any("many" in r.getMessage() and "7" in r.getMessage() for r in caplog.records)
    assert X.normalise("Hello,") == "hello" and X.normalise("(rock'n'roll)") == "rock'n'roll" and X.normalise("--") is None and X.normalise("'Tis") == "tis"
    assert X.normalise_words(["A", "--", "b."]) == ["a", "b"]
    assert lex.labels(["the", "zebra"]) == ["AH0", "DH", "IY0"]
    (tmp_path / "bad.txt").write_text("THE DH AH0\nLONELY\n")
    with pytest.raises(ValueError, match=r"bad.txt:2"):
        X.read_lexicon(str(tmp_path / "bad.txt"))
    (tmp_path / "empty.txt").write_text("# nothing\n")
    with pytest.raises(ValueError, match="no pronunciations"):
        X.read_lexicon(str(tmp_path / "empty.txt"))


# ---- the word graph -------------------------------------------------------------------------------------------------------------------------------------
def lex3():
    from fcl_taco2_amd import lexicon as X

    return X.Lexicon({"the": [["dh", "ah"], ["dh", "iy"]], "cat": [["k", "ae", "t"]], "either": [["iy", "dh", "er"], ["ay", "dh", "er"], ["iy", "dh", "ah"]]})


PHONES = ["ae", "ah", "ay", "dh", "er", "iy", "k", "sil", "t"]
INDEX = {p: i for i, p in enumerate(PHONES)}


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("boundary", [True, False])
def test_word_graph_invariants(A, K, boundary):
    words = ["The", "cat,", "either", "the"]
    g = A.build_word_graph(words, lex3(), INDEX, "sil", K, boundary, "u1")
    vocab = lex3()
    ref = L.word_graph([[[INDEX[p] for p in v] for v in vocab.lookup(w)] for w in words], INDEX["sil"], K, boundary)
    for name in ("row_state", "row_pred", "row_flags", "row_phone", "row_word", "row_variant"):
        assert np.array_equal(getattr(g, name), ref[name]) and getattr(g, name).dtype == np.int32, name
    S = len(g.row_state)
    assert S == K * (4 + 3 + 9 + 4 + 3 + (2 if boundary else 0)) and g.row_pred.shape == (S, 8)
    r = np.arange(S)[:, None]
    assert (g.row_pred >= 0).all() and (r - g.row_pred >= 0).all()  # topological order: every predecessor has a lower index
    first = lambda w, v: int(np.flatnonzero((g.row_word == w) & (g.row_variant == v))[0])
    last = lambda w, v: int(np.flatnonzero((g.row_word == w) & (g.row_variant == v))[-1])
    n_var = [2, 1, 3, 2]
    start = sorted([first(0, v) for v in range(2)] + ([0] if boundary else []))
    final = sorted([last(3, v) for v in range(2)] + ([S - 1] if boundary else []))
    assert list(np.flatnonzero(g.row_flags & A.START)) == start and list(np.flatnonzero(g.row_flags & A.FINAL)) == final
    assert set(np.unique(g.row_flags)) <= {0, 1, 2, 3}
    for w in range(4):
        for v in range(n_var[w]):
            a, b = first(w, v), last(w, v)
            assert (g.row_pred[a + 1 : b + 1, 0] == 1).all() and not g.row_pred[a + 1 : b + 1, 1:].any()  # inner rows: slot 0 = 1 alone
            sil_last = a - 1 if v == 0 else first(w, 0) - 1  # the row before the word's first variant
            has_sil = sil_last >= 0 and g.row_word[sil_last] < 0
            want = ([sil_last] if has_sil else []) + ([last(w - 1, u) for u in range(n_var[w - 1])] if w > 0 else [])
            assert list(a - g.row_pred[a][: len(want)]) == want and not g.row_pred[a][len(want):].any()  # slot order: the silence, then variant order
        if w > 0:  # the first row of sil_w: the variants of w - 1 in variant order
            s0 = first(w, 0) - K
            want = [last(w - 1, u) for u in range(n_var[w - 1])]
            assert g.row_word[s0] == -1 and list(s0 - g.row_pred[s0][: len(want)]) == want and not g.row_pred[s0][len(want):].any()
    assert (g.row_phone[g.row_word < 0] == INDEX["sil"]).all() and np.array_equal(g.row_state, g.row_phone * K + np.arange(S) % K)
    # seven variants and a silence fill the eight slots
    from fcl_taco2_amd import lexicon as X

    wide = X.Lexicon({"w": [["ae"] * (i + 1) for i in range(7)], "x": [["k"]]})
    g8 = A.build_word_graph(["w", "x"], wide, INDEX, "sil", K, boundary, "u")
    assert (g8.row_pred[np.flatnonzero(g8.row_word == 1)[0]] > 0).all()


def test_canonical_chain_flat_start(A):
    K = 3
    g = A.build_word_graph(["the", "cat", "either"], lex3(), INDEX, "sil", K, True, "u")
    ref = L.word_graph([[[INDEX[p] for p in v] for v in lex3().lookup(w)] for w in ["the", "cat", "either"]], INDEX["sil"], K, True)
    full, bare = A.canonical_rows(g, True), A.canonical_rows(g, False)
    assert len(full) == K * (2 + 3 + 3 + 2) and len(bare) == K * (2 + 3 + 3) and set(bare) <= set(full)
    assert (g.row_variant[bare] == 0).all() and (g.row_word[sorted(set(full) - set(bare))] == -1).all()
    assert list(sorted(set(full) - set(bare))) == [0, 1, 2] + list(range(len(g.row_state) - 3, len(g.row_state)))
    for T, rows in ((100, full), (len(full), full), (len(full) - 1, bare), (len(bare), bare)):  # with the silences; below their count: without
        c = A.uniform_word_alignment(T, g)
        assert c.sum() == T and (c[rows] >= 1).all() and not np.delete(c, rows).any() and c.max() - c[rows].min() <= 1
        assert np.array_equal(c, L.uniform_alignment(T, ref)) and np.array_equal(c, A.flat_start(T, g))
    assert A.uniform_word_alignment(len(bare) - 1, g) is None and L.uniform_alignment(len(bare) - 1, ref) is None  # sits the flat start out
    # the chain's own flat start is untouched
    row_skip = np.asarray([0, 0, 0, 0, 0, 0, 4, 0, 0])
    assert np.array_equal(A.flat_start(20, (np.arange(9), row_skip)), R.uniform_alignment(20, row_skip))


def test_refusals_by_name(A):
    lex = lex3()
    with pytest.raises(ValueError, match="utterance u7: not in the lexicon: dog, zebra$"):
        A.build_word_graph(["the", "zebra", "dog", "Zebra"], lex, INDEX, "sil", 3, True, "u7")
    with pytest.raises(ValueError, match="utterance u7: label 'er' is not in the inventory"):
        A.build_word_graph(["either"], lex, {p: i for i, p in enumerate(PHONES) if p != "er"}, "sil", 3, True, "u7")
    with pytest.raises(ValueError, match="utterance u7: label 'sp' is not in the inventory"):
        A.build_word_graph(["the"], lex, INDEX, "sp", 3, True, "u7")
    with pytest.raises(ValueError, match="utterance u7 has an empty transcript"):
        A.build_word_graph(["--", "..."], lex, INDEX, "sil", 3, True, "u7")
    with pytest.raises(ValueError, match=r"u7.*1026 rows.*at most 1024"):
        A.build_word_graph(["cat"] * 84 + ["the"], lex, INDEX, "sil", 3, True, "u7")  # 3 x (252 + 4 labels, 84 + 2 silences)
    assert len(A.build_word_graph(["cat"] * 84 + ["the"], lex, INDEX, "sil", 3, False, "u").row_state) == 1020
    al = object.__new__(A.Aligner)
    for optional in (set(), {"sil", "sp"}):
        al.optional = optional
        with pytest.raises(ValueError, match="exactly one label"):
            al.silence()


def test_maps_carry_the_lattice_tables(A):
    g = A.build_word_graph(["the", "cat"], lex3(), INDEX, "sil", 2, True, "u")
    h = A.build_word_graph(["either"], lex3(), INDEX, "sil", 2, False, "v")
    mp = A.AlignMaps([30, 20], [g, h], len(PHONES) * 2, "cpu")
    assert mp.lattice and mp.row_pred.shape == (mp.rows, 8) and mp.max_skip == 0
    assert np.array_equal(mp.row_preds, np.concatenate([g.row_pred, h.row_pred])) and np.array_equal(mp.row_flagss, np.concatenate([g.row_flags, h.row_flags]))
    state_off, state_rows = R.state_lists(mp.row_states, mp.n_states)
    assert np.array_equal(state_off, mp.state_offs) and np.array_equal(state_rows, mp.state_rows_h)
    chain = A.AlignMaps([30], [(np.arange(4), np.zeros(4, np.int32))], 4, "cpu")
    assert not chain.lattice and not hasattr(chain, "row_pred")


# ---- the C entry ------------------------------------------------------------------------------------------------------------------------------------------
def test_entry_validates_before_any_hip_call(A):
    from fcl_taco2_amd import _lib

    lib = _lib.load()
    P = 4096  # any non-null pointer: validation returns before it is used
    assert lib.fcl_al_lattice_viterbi_fwd(None, None) == -1

    def args(**kw):
        a = _lib.AlignLattice()
        a.frames, a.rows, a.cells, a.n_utt, a.n_states, a.max_t, a.max_s = 20, 6, 60, 2, 5, 10, 3
        for f in ("ll", "frame_off", "row_off", "cell_off", "row_state", "row_pred", "row_flags", "workspace", "frame_row", "row_begin", "row_frames", "score", "ok"):
            setattr(a, f, P)
        a.workspace_bytes = 256
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for bad in (dict(max_t=4097), dict(max_s=1025), dict(max_t=0), dict(max_s=0), dict(n_states=0), dict(n_states=1025), dict(n_utt=65536), dict(n_utt=-1),
                dict(cells=0), dict(frames=0), dict(rows=0), dict(frames=1 << 40)):
        assert lib.fcl_al_lattice_viterbi_fwd(C.byref(args(**bad)), None) == -2, bad
    assert b"max_t" in (lib.fcl_al_lattice_viterbi_fwd(C.byref(args(max_t=4097)), None), lib.fcl_last_error())[1]
    for f in ("ll", "cell_off", "row_pred", "row_flags", "workspace", "frame_row", "ok"):
        assert lib.fcl_al_lattice_viterbi_fwd(C.byref(args(**{f: None})), None) == -1, f
    assert lib.fcl_al_lattice_viterbi_fwd(C.byref(args(workspace_bytes=255)), None) == -5 and b"fcl_al_workspace_bytes" in lib.fcl_last_error()
    assert lib.fcl_al_lattice_viterbi_fwd(C.byref(_lib.AlignLattice(n_utt=0, n_states=5)), None) == 0  # an empty batch launches nothing


def test_struct_layout_matches_the_header(tmp_path):
    from fcl_taco2_amd import _lib

    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fcl_hip.h"\nint main(void) {\n' + "".join(
        '  printf("%s %%zu\\n", offsetof(fcl_al_lattice_t, %s));\n' % (n, n) for n, _ in _lib.AlignLattice._fields_) +
        '  printf("sizeof %zu\\n", sizeof(fcl_al_lattice_t));\n  printf("flags %d\\n", FCL_AL_START + 10 * FCL_AL_FINAL);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict((ln.split()[0], int(ln.split()[1])) for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert out.pop("sizeof") == C.sizeof(_lib.AlignLattice) and out.pop("flags") == 21
    assert out == {n: getattr(_lib.AlignLattice, n).offset for n, _ in _lib.AlignLattice._fields_}


# ---- the trainer ------------------------------------------------------------------------------------------------------------------------------------------
def test_flat_start_fit_of_the_float64_reference_on_the_word_corpus():
    """4 rounds after the flat start on the canonical chains: at least 95 % of the multi-variant words get the variant the recording holds and the
    frame accuracy reaches 0.98 (a condition on the corpus)"""
    c = L.corpus(0)
    assert len(c["feats"]) == 60 and all(4 <= len(w) <= 9 for w, _ in c["picks"]) and len(c["vocab"]) == 20
    multi = [v for v in c["vocab"] if len(v) > 1]
    assert len(multi) == 7 and all(2 <= len(v) <= 3 and all(a != v[0] and len(a) == len(v[0]) for a in v[1:]) for v in multi)
    assert all(len(x) == len(t) for x, t in zip(c["feats"], c["truth"])) and all(len(g["row_state"]) <= 1024 for g in c["graphs"])
    mean, var, history = L.fit(c["feats"], c["graphs"], c["M"], 4)
    counts, _ = L.align(c["feats"], c["graphs"], mean, var)
    acc = R.frame_accuracy(counts, c["codes"], c["truth"])
    var_acc, n_multi = L.variant_accuracy(counts, c["graphs"], c["picks"], c["vocab"])
    print("word corpus: frame accuracy %.4f, %.4f of %d multi-variant words right, score %s" % (acc, var_acc, n_multi, ["%.3f" % s for s in history]))
    assert n_multi >= 80 and history[-1] > history[0] and all(cnt is not None for cnt in counts)
    assert var_acc >= 0.95 and acc >= 0.98
