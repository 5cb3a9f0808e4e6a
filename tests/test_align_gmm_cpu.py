"""The mixture half of the forced-alignment contract without a GPU: the float64 statement of tests/align_gmm_ref.py against itself
(vectorised against the plain loop, the clamp of comp_off, the posteriors), the host half of fcl_taco2_amd/alignment.py against it (the split rule on
hand-made states, the M-step's floors, the model file, the schedule's targets), the C entries' validation, the driver's flag refusals, and the
float64 trainer on the synthetic corpus with voices."""
import io

import numpy as np
import pytest

import align_gmm_ref as G
import align_ref as R


@pytest.fixture(scope="module")
def A():
    from fcl_taco2_amd import alignment

    return alignment


def ragged(M):
    """C_m = 1 + (5 m mod 8)"""
    return np.concatenate([[0], np.cumsum(1 + (5 * np.arange(M)) % 8)]).astype(np.int32)


# ---- the statement ------------------------------------------------------------------------------------------------------------------------------------
def test_vectorised_statement_equals_the_plain_loop():
    rng = np.random.RandomState(0)
    M, D = 19, 5
    comp_off = ragged(M)
    Gn = int(comp_off[-1])
    mean, var, w = rng.randn(Gn, D) * 2.0, rng.uniform(0.3, 2.0, (Gn, D)), rng.uniform(0.1, 1.0, Gn)
    x = rng.randn(23, D) * 2.0
    x[3], x[5], x[7] = np.nan, np.inf, -np.inf
    l = G.comp_loglik(x, *G.params32(mean, var, w))[0]
    l[9, comp_off[2]] = -np.inf  # one component alone at -inf: the others carry the state
    a, b = G.gmm_loglik(l, comp_off), G.gmm_loglik_loop(l, comp_off)
    assert np.array_equal(a, b, equal_nan=True)
    assert np.isnan(a[3]).all() and (a[5] == -np.inf).all() and (a[7] == -np.inf).all() and np.isfinite(np.delete(a, [3, 5, 7], axis=0)).all()
    one = np.flatnonzero(np.diff(comp_off) == 1)
    assert len(one) >= 2 and np.array_equal(a[:, one], l[:, comp_off[one]], equal_nan=True)  # a one-component state is l_0 itself
    # a descending comp_off and offsets far outside: every state still reads 1 .. 8 components inside [0, G)
    for bad in (comp_off[::-1].copy(), np.asarray([-(1 << 30), 5, 1 << 30, 3, 3, 0], dtype=np.int64)):
        g0, cnt = G.state_comps(bad, Gn)
        assert (g0 >= 0).all() and (cnt >= 1).all() and (cnt <= 8).all() and (g0 + cnt <= Gn).all()
    g0, cnt = G.state_comps(comp_off, Gn)
    assert np.array_equal(g0, comp_off[:-1]) and np.array_equal(cnt, np.diff(comp_off))
    assert G.state_comps(comp_off, Gn, max_comp=3)[1].max() == 3


def test_batched_recurrence_equals_align_refs():
    """viterbi_batch, which the float64 trainer aligns with, is align_ref.viterbi utterance by utterance: lengths that differ, optional phonemes, an
    utterance with too few frames, a frame of NaN"""
    c = G.corpus_voices(0)
    rng = np.random.RandomState(6)
    lls = [rng.randn(len(x), c["M"]) * 3.0 for x in c["feats"][:12]]
    lls[4] = lls[4][:5]  # fewer frames than mandatory rows
    lls[7][3] = np.nan
    got = G.viterbi_batch(lls, c["graphs"][:12])
    for ll, (row_state, row_skip), g in zip(lls, c["graphs"], got):
        want = R.viterbi(ll, row_state, row_skip)
        assert g["ok"] == want["ok"] and (g["score"] == want["score"] or not want["ok"]) and np.array_equal(g["frame_row"], want["frame_row"])
        assert np.array_equal(g["row_frames"], want["row_frames"]) and np.array_equal(g["row_begin"], want["row_begin"])
    assert [g["ok"] for g in got][4] == 0 and sum(g["ok"] for g in got) >= 10
    mean, var = rng.randn(c["M"], c["D"]), rng.uniform(0.5, 2.0, (c["M"], c["D"]))
    counts = G.align(c["feats"][:12], c["graphs"][:12], mean, var, np.ones(c["M"]), np.arange(c["M"] + 1))[0]
    assert all(np.array_equal(a, b) for a, b in zip(counts, R.align(c["feats"][:12], c["graphs"][:12], mean, var)[0]))


def test_consequences_of_the_contract_in_float64():
    """two equal components of weight 0.5 are the single Gaussian; a component 200 below its neighbour leaves the neighbour's value; posteriors"""
    rng = np.random.RandomState(1)
    D = 6
    mean, var = rng.randn(1, D), rng.uniform(0.5, 2.0, (1, D))
    x = rng.randn(11, D)
    single = R.loglik(x, mean, 1.0 / var, R.gconst(var))[0]
    l = G.comp_loglik(x, np.repeat(mean, 2, axis=0), np.repeat(1.0 / var, 2, axis=0), np.log([0.5, 0.5]) + np.repeat(R.gconst(var), 2))[0]
    assert np.allclose(G.gmm_loglik(l, [0, 2]), single, rtol=0, atol=1e-12)
    l[:, 1] = l[:, 0] - 200.0
    assert np.allclose(G.gmm_loglik(l, [0, 2])[:, 0], l[:, 0], rtol=0, atol=1e-15)
    assert np.array_equal(G.gmm_loglik(l.astype(np.float32).astype(np.float64), [0, 2])[:, 0].astype(np.float32), l[:, 0].astype(np.float32))
    comp_off = ragged(5)
    lg = rng.randn(11, int(comp_off[-1])) * 3.0
    fs = np.asarray([0, 1, 2, 3, 4, -1, 7, 0, 1, 2, -1])  # 7: above M - 1, counts as 4
    gamma, arg, cnt = G.posteriors(lg, comp_off, fs)
    assert gamma.shape == (11, 8) and not gamma[fs < 0].any() and np.allclose(gamma[fs >= 0].sum(axis=1), 1.0)
    assert np.array_equal(gamma[0], np.eye(8)[0]) and np.array_equal(gamma[6], G.posteriors(lg[6:7], comp_off, [4])[0][0])
    for f in np.flatnonzero(fs >= 0):
        m = min(fs[f], 4)
        v = lg[f, comp_off[m] : comp_off[m + 1]]
        assert np.allclose(gamma[f, : len(v)], np.exp(v - v.max()) / np.exp(v - v.max()).sum()) and not gamma[f, len(v) :].any() and cnt[f] == len(v)
        assert (arg[f] <= 0).all()
    assert np.array_equal(G.frame_states([4, 2, 9], [0, 3, 3], [3, 0, 2], 7), [4, 4, 4, 9, 9, -1, -1])


def test_stats_chain_sums_to_the_single_gaussian_statistics():
    rng = np.random.RandomState(2)
    M, D, frames = 3, 4, 40
    comp_off = np.asarray([0, 2, 3, 6], dtype=np.int32)
    x = rng.randn(frames, D).astype(np.float32)
    row_state = np.asarray([0, 1, 2, 1, 0], dtype=np.int32)
    row_begin, row_frames = np.asarray([0, 9, 14, 22, 30]), np.asarray([9, 5, 8, 8, 10])
    fs = G.frame_states(row_state, row_begin, row_frames, frames)
    gamma = G.posteriors(rng.randn(frames, 6) * 2.0, comp_off, fs)[0].astype(np.float32)
    state_off, state_rows = R.state_lists(row_state, M)
    w, s, q = np.zeros(6), np.zeros((6, D)), np.zeros((6, D))
    G.stats_chain(x, gamma, row_begin, row_frames, state_off, state_rows, comp_off, w, s, q)
    n1, s1, q1 = np.zeros(M, np.int64), np.zeros((M, D)), np.zeros((M, D))
    R.stats_chain(x, row_begin, row_frames, state_off, state_rows, n1, s1, q1)
    for m in range(M):
        sl = slice(comp_off[m], comp_off[m + 1])
        assert abs(w[sl].sum() - n1[m]) <= 10 * G.U * n1[m] and np.allclose(s[sl].sum(axis=0), s1[m], atol=1e-4) and np.allclose(q[sl].sum(axis=0), q1[m], atol=1e-4)
    assert w[2] == n1[1] and np.array_equal(s[2], s1[1]) and np.array_equal(q[2], q1[1])  # a one-component state: gamma is exactly 1


# ---- the host half of the package ---------------------------------------------------------------------------------------------------------------------
def test_split_rule_on_hand_made_states(A):
    D = 2
    one = lambda v: np.full((1, D), float(v))
    for fn in (A.split_components, G.split_to):
        # a plain split: weight and occupancy halved, + 0.2 sigma kept in place, - 0.2 sigma appended
        mean, var, w, occ, off = fn(one(1.0), one(4.0), [1.0], [40.0], [0, 1], 2, 10.0)
        assert list(off) == [0, 2] and np.allclose(mean, [[1.4] * D, [0.6] * D]) and np.array_equal(var, [[4.0] * D] * 2) and list(w) == [0.5, 0.5] and list(occ) == [20.0, 20.0]
        # ties: the first of the equal weights is split, the copy goes to the END of the state's list
        mean, var, w, occ, off = fn(np.asarray([[0.0] * D, [10.0] * D]), np.ones((2, D)), [0.5, 0.5], [30.0, 30.0], [0, 2], 3, 10.0)
        assert list(off) == [0, 3] and np.allclose(mean[:, 0], [0.2, 10.0, -0.2]) and list(w) == [0.25, 0.5, 0.25]
        # ... and the next split takes the component of largest weight, the second
        mean, var, w, occ, off = fn(np.asarray([[0.0] * D, [10.0] * D]), np.ones((2, D)), [0.5, 0.5], [30.0, 30.0], [0, 2], 4, 10.0)
        assert np.allclose(mean[:, 0], [0.2, 10.2, -0.2, 9.8]) and list(w) == [0.25, 0.25, 0.25, 0.25] and list(occ) == [15.0] * 4
        # an occupancy just below 2 min_occupancy: no split; just at it: split
        assert list(fn(one(0.0), one(1.0), [1.0], [19.999], [0, 1], 2, 10.0)[4]) == [0, 1]
        assert list(fn(one(0.0), one(1.0), [1.0], [20.0], [0, 1], 2, 10.0)[4]) == [0, 2]
        # a target the state cannot reach: 30 -> 15 + 15, and 15 is below 20: it stops at 2 of 8; the neighbour with 400 frames reaches 8; a third keeps 1
        mean, var, w, occ, off = fn(np.zeros((3, D)), np.ones((3, D)), [1.0, 1.0, 1.0], [30.0, 400.0, 3.0], [0, 1, 2, 3], 8, 10.0)
        assert list(off) == [0, 2, 10, 11] and list(occ[:2]) == [15.0, 15.0] and np.allclose(occ[2:10], 50.0) and w[10] == 1.0
        for m in range(3):
            assert abs(w[off[m] : off[m + 1]].sum() - 1.0) < 1e-15
    rng = np.random.RandomState(4)
    args = (rng.randn(7, 3), rng.uniform(0.5, 2.0, (7, 3)), [0.3, 0.7, 1.0, 0.2, 0.2, 0.6, 1.0], rng.uniform(5, 200, 7), [0, 2, 3, 6, 7], 5, 10.0)
    assert all(np.array_equal(a, b) for a, b in zip(A.split_components(*args), G.split_to(*args)))
    assert [A.mixture_targets(n) for n in range(1, 9)] == [[], [2], [2, 3], [2, 4], [2, 4, 5], [2, 4, 6], [2, 4, 7], [2, 4, 8]]
    assert all(A.mixture_targets(n) == G.targets(n) for n in range(1, 9))


def test_mstep_floors_kept_components_and_weight_floor(A):
    rng = np.random.RandomState(3)
    D = 4
    comp_off = np.asarray([0, 3, 5, 6], dtype=np.int32)
    # state 0: a spread component, a constant one (floored), one with w < 2 (kept); state 1: occupancy below 2 (weights kept); state 2: one component
    x = [rng.randn(60, D) * 3.0, np.ones((8, D)) * 2.0, rng.randn(1, D), rng.randn(1, D) * 0.5, np.zeros((0, D)), rng.randn(30, D)]
    gam = [np.full(60, 0.9), np.ones(8), np.full(1, 1e-4), np.full(1, 0.7), np.zeros(0), np.ones(30)]
    w = np.asarray([g.sum() for g in gam])
    s, q = np.stack([(g[:, None] * v).sum(axis=0) for g, v in zip(gam, x)]), np.stack([(g[:, None] * v * v).sum(axis=0) for g, v in zip(gam, x)])
    mean0, var0, weight0 = rng.randn(6, D), rng.rand(6, D) + 0.5, np.asarray([0.5, 0.3, 0.2, 0.6, 0.4, 1.0])
    N = w.sum()
    floor = 0.01 * (q.sum(axis=0) / N - (s.sum(axis=0) / N) ** 2)
    for fn in (A.mstep_mixtures, G.mstep):
        mean, var, weight = fn(w, s, q, mean0, var0, weight0, comp_off)
        assert np.allclose(mean[0], x[0].mean(axis=0)) and np.allclose(var[0], x[0].var(axis=0)) and (var[0] > floor).all()
        assert np.allclose(mean[1], 2.0) and np.allclose(var[1], floor, rtol=1e-9)
        assert np.array_equal(mean[2:5], mean0[2:5]) and np.array_equal(var[2:5], var0[2:5])  # w < 2: kept
        occ = w[:3].sum()
        want = np.maximum(w[:3] / occ, 1e-5)
        assert weight[2] == pytest.approx(1e-5, rel=1e-3) and np.allclose(weight[:3], want / want.sum()) and abs(weight[:3].sum() - 1.0) < 1e-15
        assert np.array_equal(weight[3:5], weight0[3:5]) and weight[5] == 1.0  # occupancy 0.7: kept
    assert all(np.array_equal(a, b) for a, b in zip(A.mstep_mixtures(w, s, q, mean0, var0, weight0, comp_off), G.mstep(w, s, q, mean0, var0, weight0, comp_off)))
    # with one component everywhere the mixture M-step is the single-Gaussian one
    n = np.asarray([50.0, 6.0, 1.0])
    s3, q3 = rng.randn(3, D) * n[:, None], (rng.rand(3, D) + 2.0) * n[:, None]
    m1, v1 = A.mstep(n, s3, q3, mean0[:3], var0[:3])
    m2, v2, w2 = A.mstep_mixtures(n, s3, q3, mean0[:3], var0[:3], np.ones(3), np.arange(4))
    assert np.array_equal(m1, m2) and np.array_equal(v1, v2) and list(w2) == [1.0, 1.0, 1.0]


def test_model_file_round_trip(A, tmp_path):
    rng = np.random.RandomState(5)
    phones, K, D = ["a", "b"], 2, 3
    # today's file: a one-component model writes exactly what it always wrote, and loads as one component per state
    m = A.AlignModel(phones, K, rng.randn(4, D), rng.rand(4, D) + 0.5, dict(fs=22050, hop=256))
    m.save(str(tmp_path / "one.npz"))
    import json

    buf = io.BytesIO()
    np.savez(buf, phones=np.asarray(m.phones), states=np.int64(m.K), mean=m.mean, var=m.var, settings=np.asarray(json.dumps(m.settings, sort_keys=True)))
    assert (tmp_path / "one.npz").read_bytes() == buf.getvalue()
    z = A.AlignModel.load(str(tmp_path / "one.npz"))
    assert not z.is_mixture and z.n_states == 4 and z.n_components == 4 and z.max_components == 1 and list(z.comp_off) == [0, 1, 2, 3, 4] and list(z.weight) == [1.0] * 4
    assert all(np.array_equal(a, b) for a, b in zip(z.params32(), R.params32(m.mean, m.var)))
    # one component per state given as a mixture is the same file again
    A.AlignModel(phones, K, m.mean, m.var, m.settings, weight=np.ones(4), comp_off=np.arange(5)).save(str(tmp_path / "one2.npz"))
    assert (tmp_path / "one2.npz").read_bytes() == buf.getvalue()
    # mixtures
    comp_off = np.asarray([0, 2, 3, 6, 7])
    weight = np.asarray([0.25, 0.75, 1.0, 0.2, 0.3, 0.5, 1.0])
    g = A.AlignModel(phones, K, rng.randn(7, D), rng.rand(7, D) + 0.5, dict(fs=22050), weight=weight, comp_off=comp_off)
    g.save(str(tmp_path / "mix.npz"))
    with np.load(str(tmp_path / "mix.npz")) as f:
        assert sorted(f.files) == ["comp_off", "mean", "phones", "settings", "states", "var", "weight"] and f["comp_off"].dtype == np.int32
    z = A.AlignModel.load(str(tmp_path / "mix.npz"))
    assert z.is_mixture and z.n_states == 4 and z.n_components == 7 and z.max_components == 3 and z.dim == D and z.settings == dict(fs=22050)
    assert np.array_equal(z.mean, g.mean) and np.array_equal(z.var, g.var) and np.array_equal(z.weight, weight) and np.array_equal(z.comp_off, comp_off)
    mean32, ivar32, cc32, off = z.gmm_params32()
    want = G.params32(g.mean, g.var, weight)
    assert all(a.dtype == np.float32 and np.array_equal(a, b) for a, b in zip((mean32, ivar32, cc32), want)) and off.dtype == np.int32
    for bad in (dict(weight=weight), dict(weight=weight, comp_off=[0, 2, 3, 6]), dict(weight=weight, comp_off=[0, 2, 2, 6, 7]), dict(weight=-weight, comp_off=comp_off),
                dict(weight=weight[:6], comp_off=comp_off)):
        with pytest.raises(ValueError):
            A.AlignModel(phones, K, g.mean, g.var, **bad)
    with pytest.raises(ValueError, match="1 .. 8 components"):
        A.AlignModel(["a"], 1, np.zeros((9, D)), np.ones((9, D)), weight=np.full(9, 1 / 9.0), comp_off=[0, 9])
    with pytest.raises(ValueError, match=r"\[4 states\]"):
        A.AlignModel(phones, K, np.zeros((3, D)), np.ones((3, D)))


# ---- the C entries ------------------------------------------------------------------------------------------------------------------------------------
def test_entries_validate_before_any_hip_call(A):
    from fcl_taco2_amd import _lib

    lib = _lib.load()
    P = 4096  # any non-null pointer: validation returns before it is used
    ll = lambda **k: lib.fcl_al_gmm_loglik_fwd(*[k.get(n, P) for n in ("x", "mean", "ivar", "cconst", "comp_off", "ll")], k.get("frames", 10), k.get("d", 4),
                                               k.get("m", 4), k.get("g", 8), k.get("c", 2), None)
    post = lambda **k: lib.fcl_al_gmm_post_fwd(*[k.get(n, P) for n in ("x", "mean", "ivar", "cconst", "comp_off", "frame_state", "gamma")], k.get("frames", 10),
                                               k.get("d", 4), k.get("m", 4), k.get("g", 8), k.get("c", 2), None)
    stats = lambda **k: lib.fcl_al_gmm_stats_fwd(*[k.get(n, P) for n in ("x", "gamma", "row_begin", "row_frames", "state_off", "state_rows", "comp_off", "acc_w",
                                                                          "acc_s", "acc_q")], k.get("frames", 10), k.get("rows", 3), k.get("d", 4), k.get("m", 4),
                                                 k.get("g", 8), k.get("c", 2), None)
    for fn in (ll, post, stats):
        for bad in (dict(d=0), dict(d=41), dict(m=0), dict(m=1025), dict(c=0), dict(c=9), dict(g=3), dict(g=9), dict(m=1024, g=8193, c=8), dict(frames=-1)):
            assert fn(**bad) == -2, bad
        assert fn(m=1024, g=8192, c=8, frames=0) == 0 and fn(x=None) == -1 and fn(comp_off=None) == -1 and b"null" in lib.fcl_last_error()
    assert b"max_comp" in (ll(c=9), lib.fcl_last_error())[1]
    assert ll(ll=None) == -1 and post(frame_state=None) == -1 and post(gamma=None) == -1 and stats(acc_w=None) == -1 and stats(gamma=None) == -1
    assert ll(frames=1 << 30, m=4) == -2 and stats(rows=-1) == -2
    # an empty batch: nothing to do, whatever the pointers
    assert lib.fcl_al_gmm_loglik_fwd(None, None, None, None, None, None, 0, 4, 4, 8, 2, None) == 0
    assert lib.fcl_al_gmm_post_fwd(None, None, None, None, None, None, None, 0, 4, 4, 8, 2, None) == 0
    assert lib.fcl_al_gmm_stats_fwd(None, None, None, None, None, None, None, None, None, None, 0, 0, 4, 4, 8, 2, None) == 0
    assert stats(rows=0, x=None) == 0


# ---- the driver's flags -----------------------------------------------------------------------------------------------------------------------------------
def test_driver_refuses_flags_out_of_range(tmp_path, capsys):
    from fcl_taco2_amd import align as drv

    (tmp_path / "t.txt").write_text("u a b\n")
    base = ["--wav-dir", str(tmp_path), "--transcripts", str(tmp_path / "t.txt"), "--textgrid-out", str(tmp_path / "tg")]
    args = drv.parse_args(base)
    assert args.mixtures == 1 and args.mix_iterations == 4 and args.min_occupancy == 10.0
    args = drv.parse_args(base + ["--mixtures", "8", "--mix-iterations", "0", "--min-occupancy", "1"])
    assert args.mixtures == 8 and args.mix_iterations == 0 and args.min_occupancy == 1.0
    for flags, msg in ((["--mixtures", "0"], "--mixtures must lie in 1 .. 8"), (["--mixtures", "9"], "--mixtures must lie in 1 .. 8"),
                       (["--mix-iterations", "-1"], "--mix-iterations must not be negative"), (["--min-occupancy", "0.5"], "--min-occupancy must be at least 1"),
                       (["--min-occupancy", "nan"], "--min-occupancy must be at least 1")):
        with pytest.raises(SystemExit) as e:
            drv.parse_args(base + flags)
        assert e.value.code == 2 and msg in capsys.readouterr().err


# ---- the float64 trainer ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_mixtures_beat_the_single_gaussian_on_the_corpus_with_voices(seed):
    """120 utterances, D = 4, three voices per state: 6 single-Gaussian rounds, then 4 components in 4 + 4 rounds (min_occupancy 10) must beat the
    single-Gaussian frame accuracy by at least 0.03 (the prototype: 0.884 / 0.934 / 0.938 -> 0.967 / 0.989 / 0.988 on seeds 0 / 1 / 2)"""
    c = G.corpus_voices(seed)
    assert len(c["feats"]) == 120 and c["D"] == 4 and c["M"] == 39
    single, two, four, model = G.fit_voices(seed)
    print("seed %d: frame accuracy %.4f single, %.4f with 2, %.4f with 4 components (%d in all)" % (seed, single, two, four, len(model["weight"])))
    assert model["components"] == [39] * 6 + [78] * 4 + [len(model["weight"])] * 4 and 78 < len(model["weight"]) <= 156
    assert np.diff(model["comp_off"]).max() == 4 and np.allclose(np.add.reduceat(model["weight"], model["comp_off"][:-1]), 1.0)
    assert four >= single + 0.03
