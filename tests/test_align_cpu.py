"""The forced-alignment contract without a GPU: the float64 statement of tests/align_ref.py against itself (vectorised recurrence
against the plain loop, paths written by hand, the exactness of the exact cases), the host half of fcl_taco2_amd/alignment.py against it
(graphs, the equal split, the M-step, the refusals), the C entries' validation and struct layout, the TextGrid round trip, and the flat-start
fit of the float64 trainer on the synthetic corpus."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import align_ref as R
from conftest import ROOT


@pytest.fixture(scope="module")
def A():
    from fcl_taco2_amd import alignment

    return alignment


def same(a, b):
    return (a["ok"] == b["ok"] and a["score"] == b["score"] and np.array_equal(a["frame_row"], b["frame_row"]) and np.array_equal(a["row_begin"], b["row_begin"])
            and np.array_equal(a["row_frames"], b["row_frames"]))


# ---- the recurrence -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
def test_vectorised_recurrence_equals_the_plain_loop(kind):
    for S, T in [s for s in R.SIZES if s[0] * s[1] <= 600] + [(12, 30), (30, 33)]:
        row_state, row_skip = R.case_graph(S)
        if S == 30:
            row_skip = row_skip.copy()
            row_skip[[8, 20]] = 4
        ll = R.case_ll(S, T, kind)
        a, b = R.viterbi_loop(ll, row_state, row_skip), R.viterbi(ll, row_state, row_skip)
        assert same(a, b), (S, T)
        assert a["ok"] == (0 if (S, T) == (3, 2) else 1)
        if a["ok"]:
            assert R.path_valid(a["frame_row"], row_skip) and a["row_frames"].sum() == T
            assert abs(R.path_score(ll, row_state, a["frame_row"])[0] - a["score"]) <= 1e-9 * abs(a["score"])


def test_paths_written_by_hand():
    st3, no_skip = np.arange(3), np.zeros(3, dtype=np.int32)
    # all ties: stay wins wherever its cell can be reached, so the backtrack stays in the last row as long as that row is reachable
    r = R.viterbi_loop(np.zeros((5, 3)), st3, no_skip)
    assert r["ok"] and list(r["frame_row"]) == [0, 1, 2, 2, 2] and list(r["row_frames"]) == [1, 1, 3] and list(r["row_begin"]) == [0, 1, 2] and r["score"] == 0.0
    # advance only when strictly greater: row 1 is better from frame 1 on
    ll = np.zeros((4, 3))
    ll[1:, 1] = 1.0
    ll[3, 2] = 0.5
    r = R.viterbi_loop(ll, st3, no_skip)
    assert list(r["frame_row"]) == [0, 1, 1, 2] and r["score"] == 2.5
    # a tie between advance and skip: advance holds; with the skipped row made worse the skip wins
    skip = np.asarray([0, 0, 2], dtype=np.int32)
    ll = np.zeros((3, 3))
    ll[1, 2] = -5.0  # staying in row 2 is worse than entering it in the last frame
    r = R.viterbi_loop(ll, st3, skip)
    assert list(r["frame_row"]) == [0, 1, 2] and r["score"] == 0.0
    ll[:, 1] = -1.0
    r = R.viterbi_loop(ll, st3, skip)
    assert list(r["frame_row"]) == [0, 0, 2] and list(r["row_frames"]) == [2, 0, 1] and list(r["row_begin"]) == [0, 2, 2] and r["score"] == 0.0
    # a forced skip: K = 1, S = 3, T = 2
    r = R.viterbi_loop(np.asarray([[1.0, 50.0, 2.0], [3.0, 50.0, 4.0]]), st3, skip)
    assert r["ok"] and list(r["frame_row"]) == [0, 2] and r["score"] == 5.0 and list(r["row_frames"]) == [1, 0, 1]
    # a forbidden skip: the same without row_skip has no path, and a row_skip that points before row 0 or is out of range counts as 0
    for bad in (no_skip, np.asarray([0, 2, 0]), np.asarray([0, 0, 5]), np.asarray([0, 0, 1]), np.asarray([0, 0, 3])):
        r = R.viterbi_loop(np.asarray([[1.0, 50.0, 2.0], [3.0, 50.0, 4.0]]), st3, bad)
        assert r["ok"] == 0 and r["score"] == -np.inf and list(r["frame_row"]) == [-1, -1] and not r["row_frames"].any()
    # non-finite inputs: no path, or a valid one
    ll = np.zeros((4, 3))
    ll[2, :] = np.nan
    r = R.viterbi(ll, st3, no_skip)
    assert r["ok"] == 0 or R.path_valid(r["frame_row"], no_skip)


def test_exact_cases_agree_in_float32_and_float64():
    """integer features, ivar 1, gconst 0: every value and every partial sum is exact in float32, so the float32 recurrence (what the kernel runs)
    and the float64 one give the same path and the same score -- why the GPU test may demand bit-identity on them"""
    n = 0
    for K in (1, 2, 3):
        for seed in range(12):
            S, T = K * (3 + seed % 5), 9 + 2 * seed + (seed % 3)
            ll, row_state, row_skip = R.exact_case(S, T, K, 100 * K + seed)
            a, b = R.viterbi(ll, row_state, row_skip, dtype=np.float32), R.viterbi(ll, row_state, row_skip)
            assert same(a, b)
            if a["ok"]:
                assert a["score"].dtype == np.float32 and float(a["score"]) == R.path_score(ll, row_state, a["frame_row"])[0]
            n += a["ok"]
    assert n >= 30


# ---- the host half of the package ---------------------------------------------------------------------------------------------------------------------
def test_graph_and_uniform_alignment(A):
    index = {p: i for i, p in enumerate(["a", "b", "sp"])}
    for K in (1, 2, 3):
        got = A.build_graph(["a", "sp", "b", "a"], index, {"sp"}, K, "u1")
        want = R.graph([0, 2, 1, 0], [False, True, False, False], K)
        assert all(np.array_equal(g, w) and g.dtype == np.int32 for g, w in zip(got, want))
        assert got[1][2 * K] == K + 1 and got[1].sum() == K + 1
        assert np.array_equal(A.optional_rows(got[1]), R.optional_rows(want[1])) and A.optional_rows(got[1]).sum() == K
    _, row_skip, _ = R.graph([0, 2, 1], [False, True, False], 3)
    for T in range(1, 40):
        a, b = A.uniform_alignment(T, row_skip), R.uniform_alignment(T, row_skip)
        if T < 6:
            assert a is None and b is None
            continue
        assert np.array_equal(a, b) and a.sum() == T and a.max() - a[a > 0].min() <= 1
        assert (a[3:6] == 0).all() and (a[[0, 1, 2, 6, 7, 8]] >= 1).all() if T < 9 else (a >= 1).all()
    assert list(A.uniform_alignment(7, np.zeros(3, np.int32))) == [2, 2, 3]


def test_mstep_floors_and_kept_states(A):
    rng = np.random.RandomState(3)
    M, D = 4, 5
    x = [rng.randn(50, D) * 3.0, np.ones((6, D)) * 2.0, rng.randn(1, D), np.zeros((0, D))]  # spread; constant: floored; one frame and none: kept
    n = np.asarray([len(v) for v in x])
    s, q = np.stack([v.sum(axis=0) for v in x]), np.stack([(v * v).sum(axis=0) for v in x])
    mean0, var0 = rng.randn(M, D), rng.rand(M, D) + 0.5
    allx = np.concatenate(x)
    floor = 0.01 * allx.var(axis=0)
    for fn in (A.mstep, R.mstep):
        mean, var = fn(n, s, q, mean0, var0)
        assert np.allclose(mean[0], x[0].mean(axis=0)) and np.allclose(var[0], x[0].var(axis=0)) and (var[0] > floor).all()
        assert np.allclose(mean[1], 2.0) and np.allclose(var[1], floor, rtol=1e-9)
        assert np.array_equal(mean[2:], mean0[2:]) and np.array_equal(var[2:], var0[2:])
    assert all(np.array_equal(a, b) for a, b in zip(A.mstep(n, s, q, mean0, var0), R.mstep(n, s, q, mean0, var0)))
    gm, gv = A.global_model(n, s, q, M)
    assert np.allclose(gm, allx.mean(axis=0)) and np.allclose(gv, allx.var(axis=0)) and gm.shape == (M, D)
    assert np.allclose(A.gconst(var0), R.gconst(var0)) and np.allclose(R.gconst(np.ones((1, 2))), -np.log(2 * np.pi))


def test_refusals_by_name(A, tmp_path):
    index = {p: i for i, p in enumerate(["a", "b", "sp"])}
    with pytest.raises(ValueError, match="utterance u7: label 'zz' is not in the inventory"):
        A.build_graph(["a", "zz"], index, {"sp"}, 3, "u7")
    with pytest.raises(ValueError, match="u7.*'sp' is the first label"):
        A.build_graph(["sp", "a", "b"], index, {"sp"}, 3, "u7")
    with pytest.raises(ValueError, match="u7.*'sp' is the last label"):
        A.build_graph(["a", "b", "sp"], index, {"sp"}, 3, "u7")
    with pytest.raises(ValueError, match="u7.*next to each other"):
        A.build_graph(["a", "sp", "sp", "b"], index, {"sp"}, 3, "u7")
    with pytest.raises(ValueError, match="u7.*1026 rows.*at most 1024"):
        A.build_graph(["a"] * 342, index, {"sp"}, 3, "u7")
    assert len(A.build_graph(["a"] * 1024, index, set(), 1, "u")[0]) == 1024
    with pytest.raises(ValueError, match="empty transcript"):
        A.build_graph([], index, set(), 3, "u7")
    with pytest.raises(ValueError, match="--states"):
        A.check_inventory(["a"], 4)
    with pytest.raises(ValueError, match="exceed 1024 model states"):
        A.check_inventory(["p%d" % i for i in range(342)], 3)
    from fcl_taco2_amd import _lib

    with pytest.raises(_lib.FclError, match="no CPU fallback"):
        A.Aligner("cpu", ["a", "b"])
    # the features' own checks, by the utterance's id
    import torch

    assert A.check_features([torch.zeros(5, 4), torch.zeros(4096, 4)]) == ([5, 4096], 4)
    with pytest.raises(ValueError, match="utterance long has 4097 frames; the alignment covers 1 .. 4096"):
        A.check_features([torch.zeros(5, 4), torch.zeros(4097, 4)], ["short", "long"])
    with pytest.raises(ValueError, match="utterance #1: features"):
        A.check_features([torch.zeros(5, 4), torch.zeros(5, 3)])
    with pytest.raises(ValueError, match="utterance wide: features"):
        A.check_features([torch.zeros(5, 41)], ["wide"])
    # the model file
    m = A.AlignModel(["a", "b"], 2, np.zeros((4, 3)), np.ones((4, 3)), dict(fs=22050, hop=256))
    m.save(str(tmp_path / "m.npz"))
    z = A.AlignModel.load(str(tmp_path / "m.npz"))
    assert z.phones == ["a", "b"] and z.K == 2 and np.array_equal(z.var, m.var) and z.settings == m.settings and z.n_states == 4 and z.dim == 3
    mean32, ivar32, g32 = z.params32()
    assert all(a.dtype == np.float32 for a in (mean32, ivar32, g32)) and all(np.array_equal(a, b) for a, b in zip((mean32, ivar32, g32), R.params32(m.mean, m.var)))
    with pytest.raises(ValueError, match="positive finite variances"):
        A.AlignModel(["a"], 1, np.zeros((1, 3)), np.zeros((1, 3)))
    with pytest.raises(ValueError, match=r"\[4 states\]"):
        A.AlignModel(["a", "b"], 2, np.zeros((3, 3)), np.ones((3, 3)))


def test_batches_by_cells(A):
    T, S = [100, 200, 50, 4096, 10], [10, 10, 10, 1024, 10]
    assert A.utt_batches(T, S, 3000) == [[0, 1], [2], [3], [4]]
    assert A.utt_batches(T, S, 1 << 30) == [[0, 1, 2, 3, 4]]
    assert A.utt_batches([4096] * 3, [5] * 3, 1 << 30, n_states=1 << 16) == [[0], [1], [2]]


# ---- the C entries ------------------------------------------------------------------------------------------------------------------------------------
def test_entries_validate_before_any_hip_call(A):
    from fcl_taco2_amd import _lib

    lib = _lib.load()
    P = 4096  # any non-null pointer: validation returns before it is used
    assert lib.fcl_al_workspace_bytes(0, 0) == 0 and lib.fcl_al_workspace_bytes(1, 1) == 256 and lib.fcl_al_workspace_bytes(1024 * 4096, 1) == 1024 * 4096
    assert lib.fcl_al_loglik_fwd(P, P, P, P, P, 10, 0, 4, None) == -2 and lib.fcl_al_loglik_fwd(P, P, P, P, P, 10, 41, 4, None) == -2
    assert lib.fcl_al_loglik_fwd(P, P, P, P, P, 10, 4, 1025, None) == -2 and lib.fcl_al_loglik_fwd(P, P, P, P, P, -1, 4, 4, None) == -2
    assert lib.fcl_al_loglik_fwd(P, None, P, P, P, 10, 4, 4, None) == -1 and b"null" in lib.fcl_last_error()
    assert lib.fcl_al_loglik_fwd(None, None, None, None, None, 0, 4, 4, None) == 0  # nothing to do
    assert lib.fcl_al_stats_fwd(P, P, P, P, P, P, P, P, 10, 3, 41, 4, None) == -2 and lib.fcl_al_stats_fwd(P, P, P, P, P, P, P, P, 10, 3, 4, 0, None) == -2
    assert lib.fcl_al_stats_fwd(P, P, P, P, P, None, P, P, 10, 3, 4, 4, None) == -1
    assert lib.fcl_al_stats_fwd(None, None, None, None, None, None, None, None, 0, 0, 4, 4, None) == 0
    assert lib.fcl_al_viterbi_fwd(None, None) == -1

    def args(**kw):
        a = _lib.Align()
        a.frames, a.rows, a.cells, a.n_utt, a.n_states, a.max_t, a.max_s, a.max_skip = 20, 6, 60, 2, 5, 10, 3, 4
        for f in ("ll", "frame_off", "row_off", "cell_off", "row_state", "row_skip", "workspace", "frame_row", "row_begin", "row_frames", "score", "ok"):
            setattr(a, f, P)
        a.workspace_bytes = 256
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for bad in (dict(max_t=4097), dict(max_s=1025), dict(max_t=0), dict(n_states=0), dict(n_states=1025), dict(n_utt=65536), dict(n_utt=-1), dict(max_skip=1),
                dict(max_skip=5), dict(cells=0), dict(frames=0)):
        assert lib.fcl_al_viterbi_fwd(C.byref(args(**bad)), None) == -2, bad
    assert b"max_t" in (lib.fcl_al_viterbi_fwd(C.byref(args(max_t=4097)), None), lib.fcl_last_error())[1]
    for f in ("ll", "cell_off", "row_skip", "workspace", "frame_row", "ok"):
        assert lib.fcl_al_viterbi_fwd(C.byref(args(**{f: None})), None) == -1, f
    assert lib.fcl_al_viterbi_fwd(C.byref(args(workspace_bytes=255)), None) == -5 and b"fcl_al_workspace_bytes" in lib.fcl_last_error()
    assert lib.fcl_al_viterbi_fwd(C.byref(_lib.Align(n_utt=0, n_states=5)), None) == 0  # an empty batch launches nothing


def test_struct_layout_matches_the_header(tmp_path):
    from fcl_taco2_amd import _lib

    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fcl_hip.h"\nint main(void) {\n' + "".join(
        '  printf("%s %%zu\\n", offsetof(fcl_al_t, %s));\n' % (n, n) for n, _ in _lib.Align._fields_) + '  printf("sizeof %zu\\n", sizeof(fcl_al_t));\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict((ln.split()[0], int(ln.split()[1])) for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert out.pop("sizeof") == C.sizeof(_lib.Align)
    assert out == {n: getattr(_lib.Align, n).offset for n, _ in _lib.Align._fields_}
    assert "#define FCL_ABI_VERSION 423" in open(os.path.join(ROOT, "include", "fcl_hip.h")).read()


# ---- TextGrid -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs,hop", [(22050, 256), (16000, 200)])
def test_every_boundary_survives_the_textgrid_round_trip(fs, hop, tmp_path):
    """every boundary 0 .. 4096: written as (k hop + 0.5) / fs and read back through the reference's rule int(time fs) it is k hop again; whole
    files round-trip to the durations with the last one less by 1"""
    from fcl_taco2_amd import textgrid as TG

    rng = np.random.RandomState(fs)
    edges = list(range(0, 4097))
    durations = [1] * 4096 + [3]  # T = 4099 frames is past the aligner's limit, but the writer has none: every boundary 0 .. 4096 is in this file
    phones = ["p%d" % (i % 7) for i in range(len(durations))]
    n_samples = (sum(durations) - 1) * hop + 17
    rows = TG.frame_intervals(phones, durations, fs, hop, n_samples)
    assert rows[0][0] == 0.0 and int(rows[-1][1] * fs) == n_samples and abs(rows[-1][1] - n_samples / fs) <= 1e-12
    assert [int(a * fs) for a, _, _ in rows] == [k * hop for k in edges]
    path = str(tmp_path / "all.TextGrid")
    TG.write_textgrid(path, {"phones": rows}, rows[-1][1])
    back = TG.read_textgrid(path)["phones"]
    assert back == rows  # repr round-trips every float64
    got_phones, got = TG.alignment(back, fs, hop)
    assert got_phones == phones and got == durations[:-1] + [durations[-1] - 1]
    for trial in range(20):  # random durations, zero-length ends of hop multiples, quotes in a label
        d = [int(v) for v in rng.randint(1, 40, rng.randint(1, 30))]
        T = sum(d)
        n = (T - 1) * hop + (0 if trial % 3 == 0 else int(rng.randint(0, hop)))
        assert n // hop + 1 == T
        ph = ['say "a"' if i == 0 else "x%d" % i for i in range(len(d))]
        rows = TG.frame_intervals(ph, d, fs, hop, n)
        TG.write_textgrid(path, [("phones", rows), ("words", [(0.0, rows[-1][1], "w")])], rows[-1][1])
        tiers = TG.read_textgrid(path)
        assert sorted(tiers) == ["phones", "words"]
        gp, gd = TG.alignment(tiers["phones"], fs, hop)
        assert gp == ph and gd == d[:-1] + [d[-1] - 1] and sum(gd) == T - 1
    with pytest.raises(ValueError, match="past the end"):
        TG.frame_intervals(["a"], [10], fs, hop, 8 * hop)


# ---- the float64 trainer ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_flat_start_fit_of_the_float64_reference(seed):
    """60 synthetic utterances of 6 .. 13 phonemes, 3 states, D = 8, optional pauses absent from 30 % of their places: the flat start must reach a
    frame accuracy of 0.99 within 12 iterations (measured: above 0.999 after the first on all three seeds, so the loop stops there)"""
    c = R.corpus(seed)
    assert len(c["feats"]) == 60 and all(6 * 3 <= len(g[0]) <= 25 * 3 for g in c["graphs"]) and any(g[1].any() for g in c["graphs"])
    assert 0.2 < np.mean([len(rp) // 3 - len(np.unique(tr)) > 0 for rp, tr in zip(c["row_phone"], c["truth"])]) < 1.0  # pauses really are absent
    flat = [R.uniform_alignment(len(x), g[1]) for x, g in zip(c["feats"], c["graphs"])]
    assert R.frame_accuracy(flat, c["row_phone"], c["truth"]) < 0.9  # the equal split alone is not the answer
    accs = []

    class Reached(Exception):
        pass

    def check(it, mean, var):
        counts, _ = R.align(c["feats"], c["graphs"], mean, var)
        accs.append(R.frame_accuracy(counts, c["row_phone"], c["truth"]))
        if accs[-1] >= 0.99:
            raise Reached()

    with pytest.raises(Reached):
        R.fit(c["feats"], c["graphs"], c["M"], 12, callback=check)
    print("seed %d: frame accuracy %s" % (seed, ", ".join("%.4f" % a for a in accs)))
    assert accs[-1] >= 0.99 and len(accs) <= 12
