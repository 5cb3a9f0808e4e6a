"""The three kernels of csrc/evaluate.hip, metrics.Evaluator and the evaluate driver against the float64 numpy statement of tests/evaluate_ref.py
(DESIGN.md 6h).  Every buffer a kernel writes, the workspace included, sits between guard zones filled with a NaN bit pattern, which must survive;
every test reads the library's launch record and fails if its kernel did not run.  The statement itself, the exactness of the exact cases and the
error model are checked in test_evaluate_cpu.py."""
import contextlib
import functools
import json
import wave

import numpy as np
import pytest
import torch

import evaluate_ref as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAT32 = 0x7FC12345  # an fp32 NaN: whatever is read from an unwritten word poisons the result
U = 2.0 ** -24
CEP, DTW, PITCH = "ev_cepstra_kernel", "ev_dtw_kernel", "ev_path_pitch_kernel"


@pytest.fixture(scope="module")
def M():
    assert torch.cuda.is_available()
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib, metrics

    _lib.load()
    return metrics


@contextlib.contextmanager
def launched(*names, absent=()):
    """the launches inside run the named kernels and none of `absent` (the library's own launch record)"""
    from fcl_taco2_amd import _lib

    _lib.prof_enable(True)
    try:
        yield
        torch.cuda.synchronize()
        seen = set(_lib.prof_collect())
    finally:
        _lib.prof_enable(False)
    for n in names:
        assert n in seen, (n, sorted(seen))
    for n in absent:
        assert n not in seen, (n, sorted(seen))


class Guarded(object):
    """a device buffer of n 32-bit words between two guard zones; everything starts as the NaN pattern"""

    PAD = 8192

    def __init__(self, n, dtype=torch.float32):
        self.n = int(n)
        self.buf = torch.empty(self.n + 2 * self.PAD, dtype=dtype, device=DEV)
        self.buf.view(torch.int32).fill_(PAT32)

    @property
    def t(self):
        return self.buf[self.PAD : self.PAD + self.n]

    def set(self, a):
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(a)).reshape(-1).to(self.buf.dtype))
        return self

    def np(self):
        return self.t.cpu().numpy()

    def intact(self):
        b = self.buf.view(torch.int32)
        return bool((b[: self.PAD] == PAT32).all()) and bool((b[self.PAD + self.n :] == PAT32).all())


# ---- cepstra ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_stats", [False, True], ids=["raw", "stats"])
@pytest.mark.parametrize("N,D", [(80, 13), (80, 40), (20, 1)])
def test_cepstra_vs_float64(M, N, D, with_stats):
    """1, 2, 63, 64, 65 and 300 frames (below, at and above a workgroup's 16, a partial last workgroup): every output within
    (N + 2) 2^-24 sum_m |table[k][m] x[m]| + 2^-24 |bias_k| of float64 on the float32-rounded table and bias"""
    rng = np.random.RandomState(N + D + with_stats)
    stats = np.stack([rng.uniform(-6.0, -1.0, N), rng.uniform(0.3, 2.0, N)]) if with_stats else None
    pl = M.CepstraPlan(DEV, N, D, stats)
    t0, b0 = E.table_bias(N, D, stats)
    assert np.abs(pl.table - t0).max() <= 1e-14 and np.abs(pl.bias - b0).max() <= 1e-12
    t32, b32 = pl.table_d.cpu().numpy(), pl.bias_d.cpu().numpy()
    assert np.array_equal(t32, pl.table.astype(np.float32)) and np.array_equal(b32, pl.bias.astype(np.float32)) and (with_stats or not b32.any())
    worst = 0.0
    for frames in (1, 2, 63, 64, 65, 300):
        x = (rng.randn(frames, N) if with_stats else rng.uniform(-7.0, 1.5, (frames, N))).astype(np.float32)
        xg, cg = Guarded(frames * N).set(x), Guarded(frames * D)
        with launched(CEP):
            M.launch_cepstra(pl, xg.t, cg.t, frames)
        assert xg.intact() and cg.intact()
        got = cg.np().astype(np.float64).reshape(frames, D)
        want, absum = E.cepstra(x, t32, b32)
        share = np.abs(got - want) / E.cepstra_bound(absum, b32, N)
        assert np.isfinite(got).all() and share.max() <= 1.0, (frames, float(share.max()))
        worst = max(worst, float(share.max()))
    print("cepstra N %d D %d %s: worst share of the bound %.3f" % (N, D, "stats" if with_stats else "raw", worst))


# ---- DTW ----------------------------------------------------------------------------------------------------------------------------------------
def run_dtw(M, pairs, D, workspace_bytes=None):
    """ONE ev_dtw_kernel launch over pairs [(a, b)] on guarded buffers -> [(path [n][2], n, cost as float32, the slice's bytes)] per pair"""
    mp = M.PairMaps([len(a) for a, _ in pairs], [len(b) for _, b in pairs], DEV)
    a = Guarded(mp.frames_a * D).set(np.concatenate([a for a, _ in pairs]))
    b = Guarded(mp.frames_b * D).set(np.concatenate([b for _, b in pairs]))
    nws = mp.workspace_bytes() if workspace_bytes is None else workspace_bytes
    assert nws % 4 == 0 and (workspace_bytes is not None or nws >= mp.cells)
    ws, path = Guarded(nws // 4, torch.int32), Guarded(2 * mp.path_rows, torch.int32)
    n, cost = Guarded(mp.n_pairs, torch.int32), Guarded(mp.n_pairs)
    with launched(DTW):
        M.launch_dtw(mp, D, a.t, b.t, ws.t.view(torch.uint8), path.t.view(-1, 2), n.t, cost.t)
    assert a.intact() and b.intact() and ws.intact() and path.intact() and n.intact() and cost.intact()
    host, lens, costs = path.np().reshape(-1, 2), n.np(), cost.np()
    out = []
    for k in range(mp.n_pairs):
        sl = host[mp.path_offs[k] : mp.path_offs[k + 1]]
        assert (sl[lens[k] :] == -1).all()
        out.append((sl[: lens[k]].astype(np.int64), int(lens[k]), costs[k], sl.tobytes()))
    return out


@functools.lru_cache(maxsize=None)
def device_dtw(D, kind):
    """one single-pair launch per size of the Gaussian inputs, shared by the tests that compare them"""
    from fcl_taco2_amd import metrics

    return {size: run_dtw(metrics, [E.gaussian_pair(size, D, kind)], D)[0] for size in E.SIZES}


@pytest.mark.parametrize("kind", E.KINDS)
@pytest.mark.parametrize("D", E.ORDERS)
def test_dtw_gaussian_vs_float64(M, D, kind):
    """With gamma = 1.01 (Ta + Tb + D + 2) 2^-24: the path is a valid warping path of the returned length; the returned cost is within gamma c64(G) of
    the float64 sum c64(G) of the distances along the GPU's own path G; 0 <= c64(G) - C64 <= 2.1 gamma C64 against the float64 optimum.  (Path
    identity with float64 is not demanded: a float64 margin between two predecessors can be below float32 resolution.)"""
    worst_cost, worst_gap, same = 0.0, 0.0, 0
    for size in E.SIZES:
        ref, (path, n, cost, _) = E.reference(size, D, kind), device_dtw(D, kind)[size]
        g = E.gamma(size[0], size[1], D)
        assert n == len(path) and E.is_warping_path(path, *size), size
        cG = float(E.path_cost(ref["d"], path))
        s1, s2 = abs(float(cost) - cG) / (g * cG), (cG - ref["cost"]) / (2.1 * g * ref["cost"])
        print("dtw %s D %d %r: n %d, cost %.9g, c64(G) %.12g, C64 %.12g: shares %.3f, %.3f" % (kind, D, size, n, cost, cG, ref["cost"], s1, s2))
        assert s1 <= 1.0 and cG - ref["cost"] >= 0.0 and s2 <= 1.0, size
        worst_cost, worst_gap, same = max(worst_cost, s1), max(worst_gap, s2), same + int(np.array_equal(path, ref["path"]))
    print("dtw %s D %d: worst share of the cost bound %.3f, of the optimality bound %.3f; %d of %d paths are float64's" %
          (kind, D, worst_cost, worst_gap, same, len(E.SIZES)))


def test_dtw_exact_cases_bit_for_bit(M):
    """integer cepstra with D = 1 (test_evaluate_cpu.py shows float32 and float64 agree on them): path, length and cost are the reference's, ties
    included, one launch each and all in one"""
    cases = E.exact_cases()
    batch = run_dtw(M, [(a, b) for _, a, b in cases], 1)
    for (name, a, b), got in zip(cases, batch):
        cost, path = E.dtw(a, b)
        single = run_dtw(M, [(a, b)], 1)[0]
        for path_g, n, cost_g, raw in (got, single):
            assert n == len(path) and np.array_equal(path_g, path) and float(cost_g) == cost, name
        assert got[3] == single[3] and np.float32(got[2]).tobytes() == np.float32(single[2]).tobytes()
        if (len(a), len(b)) in E.TIES and name.startswith(("same", "apart")):
            assert [tuple(v) for v in got[0]] == E.TIES[(len(a), len(b))]


@pytest.mark.parametrize("D", E.ORDERS)
def test_batch_equals_single_pair_launches_bit_for_bit(M, D):
    """all the Gaussian pairs of both kinds through ONE launch, sizes interleaved: path (the whole slice), path_len and cost are the single launches'"""
    order = [E.SIZES[i] for i in (10, 0, 7, 4, 1, 9, 2, 8, 5, 3, 6)]
    keys = [(size, kind) for size in order for kind in E.KINDS]
    got = run_dtw(M, [E.gaussian_pair(size, D, kind) for size, kind in keys], D)
    for (size, kind), (path, n, cost, raw) in zip(keys, got):
        p1, n1, c1, raw1 = device_dtw(D, kind)[size]
        assert n == n1 and raw == raw1 and np.float32(cost).tobytes() == np.float32(c1).tobytes(), (size, kind)


def test_non_finite_cepstra_still_give_a_valid_path(M):
    """NaN and infinities in both sequences, in one strip and across two (130 rows): the path written is a valid warping path of the returned length
    inside its slice (the guard zones are checked by run_dtw), whatever the cost says"""
    rng = np.random.RandomState(2)
    pairs = []
    for Ta, Tb in ((7, 9), (130, 40), (1, 5)):
        a, b = rng.randn(Ta, 13).astype(np.float32), rng.randn(Tb, 13).astype(np.float32)
        a[rng.randint(0, Ta, 3), rng.randint(0, 13, 3)] = [np.nan, np.inf, -np.inf]
        b[rng.randint(0, Tb, 3), rng.randint(0, 13, 3)] = [np.inf, np.nan, np.nan]
        pairs.append((a, b))
    pairs.append((np.full((6, 13), np.nan, np.float32), np.full((4, 13), np.nan, np.float32)))
    for (a, b), (path, n, cost, _) in zip(pairs, run_dtw(M, pairs, 13)):
        assert n == len(path) and E.is_warping_path(path, len(a), len(b)) and not np.isfinite(cost)


def test_refusals(M):
    """Ta = 4097 is refused with -2 and nothing is launched; so is a workspace one word short (-5)"""
    from fcl_taco2_amd import _lib

    mp = M.PairMaps([4097], [3], DEV)
    z = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device=DEV)
    with launched(absent=(DTW,)):
        with pytest.raises(_lib.FclError, match="error -2.*max_ta"):
            M.launch_dtw(mp, 13, z(4097 * 13), z(3 * 13), z(mp.workspace_bytes(), torch.uint8), z(2 * mp.path_rows, torch.int32).view(-1, 2), z(1, torch.int32), z(1))
        a, b = E.gaussian_pair((63, 65), 13, "noise")
        mp = M.PairMaps([63], [65], DEV)
        with pytest.raises(_lib.FclError, match="error -5.*workspace"):
            M.launch_dtw(mp, 13, z(63 * 13), z(65 * 13), z(mp.workspace_bytes() - 4, torch.uint8), z(2 * mp.path_rows, torch.int32).view(-1, 2), z(1, torch.int32), z(1))


# ---- pitch --------------------------------------------------------------------------------------------------------------------------------------
def run_pitch(M, items):
    """ONE ev_path_pitch_kernel launch over items [(Ta, Tb, path, pa, pb)] -> (counts [n][2], sums [n] float32)"""
    mp = M.PairMaps([i[0] for i in items], [i[1] for i in items], DEV)
    path = Guarded(2 * mp.path_rows, torch.int32)
    host = np.full((mp.path_rows, 2), -1, np.int32)
    for k, it in enumerate(items):
        host[mp.path_offs[k] : mp.path_offs[k] + len(it[2])] = it[2]
    path.set(host)
    n = Guarded(mp.n_pairs, torch.int32).set(np.array([len(i[2]) for i in items], np.int32))
    pa, pb = Guarded(mp.frames_a).set(np.concatenate([i[3] for i in items])), Guarded(mp.frames_b).set(np.concatenate([i[4] for i in items]))
    counts, sums = Guarded(2 * mp.n_pairs, torch.int32), Guarded(mp.n_pairs)
    with launched(PITCH):
        M.launch_path_pitch(mp, path.t.view(-1, 2), n.t, pa.t, pb.t, counts.t.view(-1, 2), sums.t)
    assert all(g.intact() for g in (path, n, pa, pb, counts, sums)) and np.array_equal(path.np().reshape(-1, 2), host)
    return counts.np().reshape(-1, 2).copy(), sums.np().copy()


def test_pitch_reduction_over_gpu_paths(M):
    """on the GPU's paths of four pairs (1 to 810 cells: below and above the 256 threads), random cents in [6500, 11600] with unvoiced runs, all
    unvoiced, all voiced, one side unvoiced: counts exact; S within (n_vv + 3) 2^-24 S64 (each term: the difference, exact here or one rounding, the
    square, and at most n_vv - 1 non-trivial additions); batch = single runs bit for bit"""
    rng = np.random.RandomState(5)
    items = []
    for size in ((1, 1), (63, 65), (5, 300), (300, 511)):
        path = device_dtw(13, "warp")[size][0]
        for ka, kb in (("runs", "runs"), ("unvoiced", "unvoiced"), ("voiced", "voiced"), ("voiced", "unvoiced")):
            items.append((size[0], size[1], path, E.pitch_inputs(ka, size[0], rng), E.pitch_inputs(kb, size[1], rng)))
    counts, sums = run_pitch(M, items)
    worst, seen_vv = 0.0, 0
    for k, (Ta, Tb, path, pa, pb) in enumerate(items):
        vv, vuv, S = E.pitch_figures(path, pa, pb)
        assert (int(counts[k, 0]), int(counts[k, 1])) == (vv, vuv), k
        assert abs(float(sums[k]) - S) <= (vv + 3) * U * S, (k, float(sums[k]), S)
        if S:
            worst, seen_vv = max(worst, abs(float(sums[k]) - S) / ((vv + 3) * U * S)), seen_vv + 1
        c1, s1 = run_pitch(M, [items[k]]) if k % 4 == 0 or Ta == 300 else (counts[k : k + 1], sums[k : k + 1])
        assert np.array_equal(c1[0], counts[k]) and s1[0].tobytes() == sums[k].tobytes(), k
        if k % 4 == 1:
            assert (vv, vuv, float(sums[k])) == (0, 0, 0.0)
        if k % 4 == 2:
            assert (vv, vuv) == (len(path), 0)
        if k % 4 == 3:
            assert (vv, vuv, float(sums[k])) == (0, len(path), 0.0)
    print("pitch reduction: worst share of the S bound %.3f over %d sums" % (worst, seen_vv))
    assert seen_vv >= 8


# ---- Evaluator and driver -----------------------------------------------------------------------------------------------------------------------
def _write_wav(path, x, rate=22050):
    pcm = np.clip(np.rint(np.asarray(x, dtype=np.float64) * 32767.0), -32768, 32767).astype("<i2")
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(rate)
        f.writeframes(pcm.tobytes())
    return pcm.astype(np.float32) / np.float32(32768.0)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """four tiny wavs (harmonic tones with a gap) and copies with a segment repeated, as <utt>_gen.wav"""
    root = tmp_path_factory.mktemp("ev")
    ref, syn = root / "ref", root / "syn"
    ref.mkdir()
    syn.mkdir()
    rng = np.random.RandomState(8)
    ids, L, hz = ["ua", "ub", "uc", "ud"], [6000, 9001, 7100, 8000], [(110.0, 150.0), (240.0, 200.0), (330.0, 330.0), (180.0, 260.0)]
    xs, ys = {}, {}
    for u, n, h in zip(ids, L, hz):
        x = E.harmonic_with_gap(22050, n, h, rng)
        s0, s1 = int(0.2 * n), int(0.2 * n) + 1100
        xs[u] = _write_wav(ref / (u + ".wav"), x)
        ys[u] = _write_wav(syn / (u + "_gen.wav"), np.concatenate([x[:s1], x[s0:]]))
    return dict(root=root, ref=ref, syn=syn, ids=ids, xs=xs, ys=ys)


def _evaluator(M):
    from fcl_taco2_amd import features, pitch

    return M.Evaluator(DEV, extractor=features.FeatureExtractor(features.FeaturePlan(DEV)), tracker=pitch.PitchTracker(pitch.PitchPlan(DEV)))


def test_a_directory_against_itself(M, corpus):
    """MCD exactly 0, diagonal paths, F0 RMSE 0 and V/UV error 0"""
    from fcl_taco2_amd import evaluate as V

    out = corpus["root"] / "self.json"
    with launched("fx_logmel_kernel<1024>", "px_yin_kernel<1024>", CEP, DTW, PITCH):
        doc = V.main(["--ref-wav-dir", str(corpus["ref"]), "--syn-wav-dir", str(corpus["ref"]), "--out", str(out), "--verbose", "0"])
    assert json.load(open(out)) == doc and doc["n_utt"] == 4 and doc["mcd_db"] == 0.0 and doc["vuv_error"] == 0.0 and doc["f0_rmse_cents"] == 0.0
    for r, u in zip(doc["utterances"], corpus["ids"]):
        T = len(corpus["xs"][u]) // 256 + 1
        assert r == dict(id=u, ref_frames=T, syn_frames=T, path_len=T, mcd_db=0.0, f0_rmse_cents=0.0, vuv_error=0.0, n_vv=r["n_vv"]) and 5 <= r["n_vv"] < T
    ev = _evaluator(M)
    res = ev.compare_waves([corpus["xs"][u] for u in corpus["ids"]], [corpus["xs"][u] for u in corpus["ids"]], ids=corpus["ids"], return_paths=True)
    for p in res["paths"]:
        assert np.array_equal(p, np.stack([np.arange(len(p))] * 2, axis=1))


def test_repeated_segment_driver_equals_evaluator_and_float64(M, corpus):
    """the utterances against copies with 1100 samples repeated: the driver's JSON equals Evaluator.compare_waves called directly; mcd_db equals the
    float64 figure on the GPU's path and cepstra to 1e-5 relative; the cents are within 1e-2 cents of float64 1200 log2 f0 (a log2 of up to 2 ulp is
    2.2e-3 cents at 200 Hz, the product's rounding 6e-4)"""
    from fcl_taco2_amd import evaluate as V

    ids = corpus["ids"]
    out = corpus["root"] / "rep.json"
    with launched("fx_logmel_kernel<1024>", "px_yin_kernel<1024>", "px_short_run_kernel", CEP, DTW, PITCH):
        doc = V.main(["--ref-wav-dir", str(corpus["ref"]), "--syn-wav-dir", str(corpus["syn"]), "--out", str(out), "--verbose", "0"])
    ev = _evaluator(M)
    res = ev.compare_waves([corpus["xs"][u] for u in ids], [corpus["ys"][u] for u in ids], ids=ids, return_paths=True, return_cepstra=True)
    assert doc["utterances"] == V.records_of(ids, [len(corpus["xs"][u]) // 256 + 1 for u in ids], [len(corpus["ys"][u]) // 256 + 1 for u in ids], res)
    assert doc["mcd_db"] == float(np.mean(res["mcd_db"])) and doc["settings"]["order"] == 13 and doc["n_utt"] == 4
    ca, cb = res["ref_cepstra"].cpu().numpy().astype(np.float64), res["syn_cepstra"].cpu().numpy().astype(np.float64)
    oa = np.concatenate([[0], np.cumsum([len(corpus["xs"][u]) // 256 + 1 for u in ids])])
    ob = np.concatenate([[0], np.cumsum([len(corpus["ys"][u]) // 256 + 1 for u in ids])])
    for k, u in enumerate(ids):
        Ta, Tb, path = oa[k + 1] - oa[k], ob[k + 1] - ob[k], res["paths"][k]
        assert Tb == Ta + 4 or Tb == Ta + 5
        assert E.is_warping_path(path, Ta, Tb) and len(path) == res["path_len"][k] >= Tb
        want = E.mcd_db(E.path_cost(E.distances(ca[oa[k] : oa[k + 1]], cb[ob[k] : ob[k + 1]]), path), len(path))
        assert 0.0 < res["mcd_db"][k] and abs(res["mcd_db"][k] / want - 1.0) <= 1e-5, (u, res["mcd_db"][k], want)
        assert res["n_vv"][k] >= 5 and np.isfinite(res["f0_rmse_cents"][k]) and 0.0 <= res["vuv_error"][k] < 0.5
        vv, vuv, S = E.pitch_figures(path, res["ref_cents"][oa[k] : oa[k + 1]].cpu().numpy(), res["syn_cents"][ob[k] : ob[k + 1]].cpu().numpy())
        assert (vv, vuv) == (res["n_vv"][k], res["n_vuv"][k]) and res["f0_rmse_cents"][k] == pytest.approx(E.f0_rmse(S, vv), rel=1e-4, abs=1e-3)
    _, _, f0 = ev.analyse([corpus["xs"][u] for u in ids], ids=ids)
    f0 = f0.cpu().numpy()
    got = res["ref_cents"].cpu().numpy().astype(np.float64)
    assert (f0 > 0).sum() >= 20 and np.array_equal(got == 0, f0 == 0) and np.abs(got - E.cents(f0)).max() <= 1e-2 and got[f0 > 0].min() > 6000.0


def test_mel_route_equals_wav_route_within_the_cepstra_bound(M, corpus):
    """mels-ori .npy against normalised .npy with --mel-stats and --syn-normalised: no F0 fields, and the wav route's MCD within
    MCD_SCALE max_j ||eps_j|| + 2 gamma MCD, where eps_j[k] = 2 (bound_raw + bound_normalised) covers, per coefficient of a synthesised frame, both
    float32 chains and the float32 rounding of the normalised mel, of the folded table and of the bias: a distance moves by at most ||eps_j||, so
    every path's mean distance, and with it the optimum, moves by at most the largest; gamma for the two float32 recurrences"""
    from fcl_taco2_amd import evaluate as V, extract_features as X

    ids, ev = corpus["ids"], _evaluator(M)
    ra, la, _ = ev.analyse([corpus["xs"][u] for u in ids], ids=ids)
    rb, lb, _ = ev.analyse([corpus["ys"][u] for u in ids], ids=ids)
    ra, rb = ra.cpu().numpy(), rb.cpu().numpy()
    stats = np.stack([rb.astype(np.float64).mean(axis=0), rb.astype(np.float64).std(axis=0)])
    d = corpus["root"] / "mel"
    (d / "mels-ori").mkdir(parents=True)
    (d / "mels").mkdir()
    np.save(d / "mel_stats.npy", stats)
    oa, ob = np.concatenate([[0], np.cumsum(la)]), np.concatenate([[0], np.cumsum(lb)])
    normed = {}
    for k, u in enumerate(ids):
        np.save(d / "mels-ori" / (u + ".npy"), ra[oa[k] : oa[k + 1]])
        normed[u] = X.normalise(rb[ob[k] : ob[k + 1]], stats[0], stats[1])
        np.save(d / "mels" / (u + ".npy"), normed[u])
    with launched(CEP, DTW, absent=(PITCH, "fx_logmel_kernel<1024>")):
        doc = V.main(["--ref-mel-dir", str(d / "mels-ori"), "--syn-mel-dir", str(d / "mels"), "--mel-stats", str(d / "mel_stats.npy"), "--syn-normalised",
                      "--verbose", "0"])
    wav = ev.compare_waves([corpus["xs"][u] for u in ids], [corpus["ys"][u] for u in ids], ids=ids)
    t_raw, b_raw = E.table_bias(80, 13)
    t_n, b_n = E.table_bias(80, 13, stats)
    for k, (r, u) in enumerate(zip(doc["utterances"], ids)):
        assert list(r) == ["id", "ref_frames", "syn_frames", "path_len", "mcd_db"] and (r["ref_frames"], r["syn_frames"]) == (la[k], lb[k])
        eps = 2.0 * (E.cepstra_bound(E.cepstra(rb[ob[k] : ob[k + 1]], t_raw, b_raw)[1], b_raw, 80) + E.cepstra_bound(E.cepstra(normed[u], t_n, b_n)[1], b_n, 80))
        tol = E.MCD_SCALE * float(np.sqrt((eps ** 2).sum(axis=1)).max()) + 2.0 * E.gamma(la[k], lb[k], 13) * wav["mcd_db"][k]
        print("mel route %s: MCD %.6f dB, wav route %.6f dB, tolerance %.2g" % (u, r["mcd_db"], wav["mcd_db"][k], tol))
        assert abs(r["mcd_db"] - wav["mcd_db"][k]) <= tol
    assert "vuv_error" not in doc and "f0" not in doc["settings"] and doc["settings"]["syn"]["normalised"]


def test_driver_refuses_by_name(M, corpus):
    """an unpaired id and an over-long pair (4097 frames) are refused by name before anything is launched"""
    from fcl_taco2_amd import evaluate as V

    a, b = corpus["root"] / "ra", corpus["root"] / "rb"
    a.mkdir()
    b.mkdir()
    for d in (a, b):
        _write_wav(d / "ok.wav", corpus["xs"]["ua"])
    _write_wav(a / "lonely.wav", corpus["xs"]["ub"])
    with launched(absent=(CEP, DTW, "fx_logmel_kernel<1024>")):
        with pytest.raises(ValueError, match=r"first: lonely"):
            V.main(["--ref-wav-dir", str(a), "--syn-wav-dir", str(b), "--verbose", "0"])
        _write_wav(b / "lonely.wav", np.zeros(4096 * 256 + 10))
        with pytest.raises(ValueError, match="utterance lonely has 36 reference and 4097 synthesised frames"):
            V.main(["--ref-wav-dir", str(a), "--syn-wav-dir", str(b), "--verbose", "0"])
