"""The three kernels of csrc/align_gmm.hip, Aligner.fit with mixtures and the align driver's --mixtures against the float64 numpy statement of
tests/align_gmm_ref.py.  Every buffer a kernel writes sits between guard zones filled with a NaN bit pattern, which must survive;
every test reads the library's launch record and fails if its kernel did not run.  The statement itself is checked in test_align_gmm_cpu.py."""
import functools
import json
import wave

import numpy as np
import pytest
import torch

import align_gmm_ref as G
import align_ref as R
from test_gpu_align import DEV, PAT32, A, Guarded, launched  # noqa: F401  (the harness of the chain tests; A is the fixture)

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
LOGLIK, VITERBI, STATS = "al_loglik_kernel", "al_viterbi_kernel", "al_stats_kernel"
GLOGLIK, GPOST, GSTATS = "al_gmm_loglik_kernel", "al_gmm_post_kernel", "al_gmm_stats_kernel"
FRAMES = (1, 2, 63, 64, 65, 300)


def layout(kind, M):
    """comp_off [M + 1]: one component everywhere, eight everywhere, or the ragged C_m = 1 + (5 m mod 8), whose states straddle every edge of 64"""
    cnt = dict(one=np.ones(M, np.int64), eight=np.full(M, 8, np.int64), ragged=1 + (5 * np.arange(M)) % 8)[kind]
    return np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)


def random_model(rng, comp_off, D):
    """(mean, var, weight) float64: components around their state's centre, weights that sum to 1 inside a state"""
    M, Gn = len(comp_off) - 1, int(comp_off[-1])
    state = np.repeat(np.arange(M), np.diff(comp_off))
    mean = (rng.randn(M, D) * 2.0)[state] + rng.randn(Gn, D) * 0.7
    w = rng.uniform(0.2, 1.0, Gn)
    return mean, rng.uniform(0.2, 3.0, (Gn, D)), w / np.add.reduceat(w, comp_off[:-1])[state]


class Model(object):
    """the float32 parameters on the device between guard zones, and the views the launches take"""

    def __init__(self, mean32, ivar32, cc32, comp_off):
        self.host = (mean32, ivar32, cc32, np.asarray(comp_off))
        self.G, self.D, self.M = mean32.shape[0], mean32.shape[1], len(comp_off) - 1
        self.bufs = [Guarded(a.size).set(a) for a in (mean32, ivar32, cc32)] + [Guarded(len(comp_off), torch.int32).set(np.asarray(comp_off, dtype=np.int32))]
        self.views = (self.bufs[0].t.view(self.G, self.D), self.bufs[1].t.view(self.G, self.D), self.bufs[2].t, self.bufs[3].t)

    def intact(self):
        return all(b.intact() for b in self.bufs)


def run_loglik(A, model, x, max_comp=8):
    """one al_gmm_loglik_kernel launch on guarded buffers -> ll float32 [frames][M]"""
    frames = len(x)
    xg, lg = Guarded(x.size).set(x), Guarded(frames * model.M)
    with launched(GLOGLIK):
        A.launch_gmm_loglik(model.views, xg.t, lg.t, frames, max_comp)
    assert xg.intact() and lg.intact() and model.intact()
    return lg.np().reshape(frames, model.M)


def reference(model, x, comp_off=None, max_comp=8):
    """float64 on the rounded parameters -> (ll, its bound, l, q)"""
    mean32, ivar32, cc32, off = model.host
    off = off if comp_off is None else comp_off
    l, q = G.comp_loglik(x, mean32, ivar32, cc32)
    ll = G.gmm_loglik(l, off, max_comp)
    return ll, G.gmm_loglik_bound(q, l, ll, off, model.D, max_comp), l, q


# ---- log-likelihood -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 13, 28, 40])
def test_gmm_loglik_vs_float64(A, D):
    """one component everywhere and eight everywhere at M = 1, 24, 210, 1024 (the last: G = 8192), the ragged layout at M = 210, each at 1, 2, 63, 64,
    65 and 300 frames: every value within align_gmm_ref.gmm_loglik_bound of float64 on the float32-rounded parameters; with one component
    everywhere and cconst = gconst the output is bit for bit fcl_al_loglik_fwd's"""
    rng = np.random.RandomState(100 + D)
    worst = {}
    xall = (rng.randn(max(FRAMES), D) * 2.5).astype(np.float32)
    for kind, M in [("one", m) for m in (1, 24, 210, 1024)] + [("eight", m) for m in (1, 24, 210, 1024)] + [("ragged", 210)]:
        comp_off = layout(kind, M)
        mean, var, w = random_model(rng, comp_off, D)
        model = Model(*G.params32(mean, var, w), comp_off)
        assert model.G == dict(one=M, eight=8 * M, ragged=int(comp_off[-1]))[kind]
        want, bound, _, _ = reference(model, xall)
        for frames in FRAMES:
            x = xall[:frames]
            got = run_loglik(A, model, x)
            share = np.abs(got.astype(np.float64) - want[:frames]) / bound[:frames]
            assert np.isfinite(got).all() and share.max() <= 1.0, (kind, M, frames, float(share.max()))
            worst[kind] = max(worst.get(kind, 0.0), float(share.max()))
            if kind == "one":
                assert np.array_equal(model.host[2], R.params32(mean, var)[2])  # weight 1: cconst is gconst
                single = Guarded(frames * M)
                with launched(LOGLIK):
                    A.launch_loglik(model.views[:3], torch.from_numpy(x).to(DEV), single.t, frames)
                assert single.intact() and single.np().tobytes() == got.tobytes(), (M, frames)
    print("gmm loglik D %d: worst share of the bound %s" % (D, ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


def test_gmm_loglik_consequences_bit_for_bit(A):
    """a component 200 below its neighbour leaves the neighbour's value bit for bit (fcl_al_loglik_fwd on the neighbour alone); two equal components
    of weight 0.5 give l + ln 0.5 + ln 2 within the bound"""
    rng = np.random.RandomState(7)
    M, D, frames = 70, 13, 65
    mean, var = rng.randn(M, D) * 2.0, rng.uniform(0.3, 2.0, (M, D))
    x = (rng.randn(frames, D) * 2.5).astype(np.float32)
    mean32, ivar32, g32 = R.params32(mean, var)
    two = np.arange(0, 2 * M + 1, 2, dtype=np.int32)
    rep = lambda a: np.repeat(a, 2, axis=0)
    single = Guarded(frames * M)
    with launched(LOGLIK):
        A.launch_loglik(tuple(torch.from_numpy(a).to(DEV) for a in (mean32, ivar32, g32)), torch.from_numpy(x).to(DEV), single.t, frames)
    # the second component (the first in every other state) is the same Gaussian with ln w = -200
    cc = rep(g32).copy()
    low = np.arange(2 * M).reshape(M, 2)[np.arange(M), 1 - np.arange(M) % 2]
    cc[low] = (cc[low].astype(np.float64) - 200.0).astype(np.float32)
    got = run_loglik(A, Model(rep(mean32), rep(ivar32), cc, two), x)
    assert single.intact() and got.tobytes() == single.np().tobytes()
    # two equal halves
    half = Model(rep(mean32), rep(ivar32), (rep(g32).astype(np.float64) + np.log(0.5)).astype(np.float32), two)
    got = run_loglik(A, half, x).astype(np.float64)
    l, q = G.comp_loglik(x, *half.host[:3])
    want = l[:, ::2] + np.log(2.0)  # = the float64 value on the rounded cconst = fl(gconst + ln 0.5), plus ln 2
    bound = G.gmm_loglik_bound(q, l, want, two, D)
    assert (np.abs(got - want) <= bound).all() and np.abs(want - R.loglik(x, mean32, ivar32, g32)[0]).max() < 1e-5


def test_gmm_loglik_non_finite_frames_stay_alone(A):
    """a frame of NaN, of +inf and of -inf: ll is not finite in those frames (NaN, -inf, -inf: the Viterbi entry's failure path takes the
    utterance) and bit for bit the clean launch everywhere else"""
    rng = np.random.RandomState(8)
    D, frames = 13, 65
    comp_off = layout("ragged", 210)
    model = Model(*G.params32(*random_model(rng, comp_off, D)), comp_off)
    x = (rng.randn(frames, D) * 2.5).astype(np.float32)
    clean = run_loglik(A, model, x)
    bad = x.copy()
    bad[5], bad[20], bad[47] = np.nan, np.inf, -np.inf
    got = run_loglik(A, model, bad)
    rest = np.setdiff1d(np.arange(frames), [5, 20, 47])
    assert np.isnan(got[5]).all() and (got[20] == -np.inf).all() and (got[47] == -np.inf).all()
    assert np.isfinite(got[rest]).all() and got[rest].tobytes() == clean[rest].tobytes()
    one = bad.copy()
    one[20, 1:] = x[20, 1:]  # a single +inf coefficient does the same
    assert (run_loglik(A, model, one)[20] == -np.inf).all()


# ---- posteriors and statistics on Viterbi alignments -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def e_step():
    """The synthetic corpus of align_ref in two batches, the first with an utterance that has too few frames for its rows (no alignment: frame_state
    -1), under a ragged mixture model grown from the float64 reference's first single-Gaussian model: mixture log-likelihoods, Viterbi, frame_state
    by torch indexing, posteriors, and both statistics chained over the batches, everything on guarded buffers.  Shared by the tests below."""
    from fcl_taco2_amd import alignment as A

    c = R.corpus(0)
    M, D = c["M"], c["D"]
    rng = np.random.RandomState(9)
    mean1, var1 = R.fit(c["feats"], c["graphs"], M, 1)[:2]
    comp_off = layout("ragged", M)
    Gn = int(comp_off[-1])
    state = np.repeat(np.arange(M), np.diff(comp_off))
    w = rng.uniform(0.2, 1.0, Gn)
    mean, var, weight = mean1[state] + rng.randn(Gn, D) * 0.8 * np.sqrt(var1[state]), var1[state] * rng.uniform(0.6, 1.2, (Gn, D)), w / np.add.reduceat(w, comp_off[:-1])[state]
    model = Model(*G.params32(mean, var, weight), comp_off)
    acc = [Guarded(Gn, torch.float64).set(np.zeros(Gn)), Guarded(Gn * D, torch.float64).set(np.zeros(Gn * D)), Guarded(Gn * D, torch.float64).set(np.zeros(Gn * D))]
    acc1 = [Guarded(M, torch.int64).set(np.zeros(M, np.int64)), Guarded(M * D, torch.float64).set(np.zeros(M * D)), Guarded(M * D, torch.float64).set(np.zeros(M * D))]
    batches = []
    for lo, hi in ((0, 37), (37, 60)):
        feats, graphs = list(c["feats"][lo:hi]), list(c["graphs"][lo:hi])
        if lo == 0:
            feats.insert(5, c["feats"][3][:7])  # 7 frames for at least 18 mandatory rows
            graphs.insert(5, c["graphs"][3])
        mp = A.AlignMaps([len(v) for v in feats], graphs, M, DEV)
        x = np.concatenate(feats)
        xg, ll = Guarded(x.size).set(x), Guarded(mp.frames * M)
        ws = torch.empty(mp.workspace_bytes(), device=DEV, dtype=torch.uint8)
        frame_row, row_begin, row_frames = Guarded(mp.frames, torch.int32), Guarded(mp.rows, torch.int32), Guarded(mp.rows, torch.int32)
        score, ok, gamma = Guarded(mp.n_utt), Guarded(mp.n_utt, torch.int32), Guarded(mp.frames * 8)
        with launched(GLOGLIK, VITERBI, GPOST, GSTATS, STATS):
            A.launch_gmm_loglik(model.views, xg.t, ll.t, mp.frames)
            A.launch_viterbi(mp, ll.t, ws, frame_row.t, row_begin.t, row_frames.t, score.t, ok.t)
            fs = A.frame_states(mp, frame_row.t)
            A.launch_gmm_post(model.views, xg.t, fs, gamma.t, mp.frames)
            A.launch_gmm_stats(mp, model.views[3], xg.t, gamma.t, row_begin.t, row_frames.t, acc[0].t, acc[1].t.view(Gn, D), acc[2].t.view(Gn, D))
            A.launch_stats(mp, xg.t, row_begin.t, row_frames.t, acc1[0].t, acc1[1].t.view(M, D), acc1[2].t.view(M, D))
        assert all(g.intact() for g in [xg, ll, frame_row, row_begin, row_frames, score, ok, gamma] + acc + acc1) and model.intact()
        batches.append(dict(mp=mp, x=x, fs=fs.cpu().numpy(), gamma=gamma.np().reshape(-1, 8), row_begin=row_begin.np(), row_frames=row_frames.np(), ok=ok.np(),
                            frame_row=frame_row.np()))
    return dict(c=c, model=model, comp_off=comp_off, batches=batches, acc=[a.np() for a in acc], acc1=[a.np() for a in acc1])


def test_posteriors_vs_float64(A):
    """gamma within align_gmm_ref.posterior_bound of float64; exactly 0 for frame_state -1 and beyond the state's count, exactly 1 for one-component
    states; sum_c gamma within (C + 2) U of 1; frame_state by torch indexing is what the rows say"""
    e = e_step()
    model, comp_off = e["model"], e["comp_off"]
    cnt_m = np.diff(comp_off)
    worst, seen_one, seen_none = 0.0, 0, 0
    for k, b in enumerate(e["batches"]):
        mp, fs, got = b["mp"], b["fs"], b["gamma"]
        assert fs.dtype == np.int32 and np.array_equal(fs, G.frame_states(mp.row_states, b["row_begin"], b["row_frames"], mp.frames))
        assert (b["ok"] == 0).sum() == (1 if k == 0 else 0) and ((fs < 0).sum() == 7) == (k == 0)
        l, q = G.comp_loglik(b["x"], *model.host[:3])
        want, arg, cnt = G.posteriors(l, comp_off, fs)
        lb = R.loglik_bound(q, l, model.D)
        m = np.clip(fs, 0, model.M - 1)
        B = np.asarray([lb[f, comp_off[m[f]] : comp_off[m[f] + 1]].max() for f in range(mp.frames)])
        bound = G.posterior_bound(want, arg, cnt, B)
        live = fs >= 0
        share = np.abs(got.astype(np.float64) - want)[live] / bound[live]
        assert share.max() <= 1.0, float(share.max())
        worst = max(worst, float(share.max()))
        assert not got[~live].any() and not got[np.arange(8)[None, :] >= cnt[:, None]].any()
        one = live & (cnt_m[m] == 1)
        assert (got[one, 0] == 1.0).all()
        assert (np.abs(got[live].astype(np.float64).sum(axis=1) - 1.0) <= (cnt[live] + 2) * U).all()
        seen_one, seen_none = seen_one + int(one.sum()), seen_none + int((~live).sum())
    assert seen_one > 50 and seen_none == 7
    print("posteriors: worst share of the bound %.3f" % worst)


def test_stats_chain_bit_for_bit_from_the_devices_own_gamma(A):
    """two batches chained: acc_w / acc_s / acc_q are bit for bit align_gmm_ref.stats_chain on the device's gamma; summed over a state's components
    they agree with fcl_al_stats_fwd on the same alignment to within the rounding of gamma's sum, (C + 2) U per frame"""
    e = e_step()
    model, comp_off, M, D = e["model"], e["comp_off"], e["model"].M, e["model"].D
    Gn = model.G
    want = [np.zeros(Gn), np.zeros((Gn, D)), np.zeros((Gn, D))]
    ax, ax2 = np.zeros((M, D)), np.zeros((M, D))
    for b in e["batches"]:
        mp = b["mp"]
        G.stats_chain(b["x"], b["gamma"], b["row_begin"], b["row_frames"], mp.state_offs, mp.state_rows_h, comp_off, *want)
        live = b["fs"] >= 0
        np.add.at(ax, b["fs"][live], np.abs(b["x"][live].astype(np.float64)))
        np.add.at(ax2, b["fs"][live], b["x"][live].astype(np.float64) ** 2)
    got_w, got_s, got_q = e["acc"][0], e["acc"][1].reshape(Gn, D), e["acc"][2].reshape(Gn, D)
    assert got_w.tobytes() == want[0].tobytes() and got_s.tobytes() == want[1].tobytes() and got_q.tobytes() == want[2].tobytes()
    n, s, q = e["acc1"][0], e["acc1"][1].reshape(M, D), e["acc1"][2].reshape(M, D)
    assert n.sum() == sum(int((b["fs"] >= 0).sum()) for b in e["batches"]) and np.abs(got_s).max() > 10.0
    for m in range(M):
        sl, tol = slice(comp_off[m], comp_off[m + 1]), (comp_off[m + 1] - comp_off[m] + 2) * U
        assert abs(got_w[sl].sum() - n[m]) <= tol * n[m] + 1e-12 * n[m], m
        assert (np.abs(got_s[sl].sum(axis=0) - s[m]) <= tol * ax[m] + 1e-12 * ax[m]).all(), m
        assert (np.abs(got_q[sl].sum(axis=0) - q[m]) <= tol * ax2[m] + 1e-12 * ax2[m]).all(), m


# ---- robustness -----------------------------------------------------------------------------------------------------------------------------------------------
def test_device_tables_the_host_cannot_check(A):
    """a comp_off that descends or points far outside, a frame_state >= M, row lists far outside their buffers: the kernels stay inside their buffers
    (the guard zones survive), read the clamped components the contract names, and leave the clean states, frames and components of the same launch
    bit for bit what the clean launch gives"""
    rng = np.random.RandomState(10)
    D, M, frames = 13, 210, 65
    comp_off = layout("ragged", M)
    Gn = int(comp_off[-1])
    params = G.params32(*random_model(rng, comp_off, D))
    model = Model(*params, comp_off)
    x = (rng.randn(frames, D) * 2.5).astype(np.float32)
    clean = run_loglik(A, model, x)
    bad = comp_off.astype(np.int64)
    bad[10:40] = bad[10:40][::-1]  # descends
    bad[60:70] = [-(1 << 30), 1 << 30, -5, Gn + 7, 0, Gn - 1, 1 << 20, -1, Gn, 3]
    bad = bad.astype(np.int32)
    untouched = np.flatnonzero((bad[:-1] == comp_off[:-1]) & (bad[1:] == comp_off[1:]))
    assert 100 < len(untouched) < M - 30
    tampered = Model(*params, bad)
    got = run_loglik(A, tampered, x)
    assert got[:, untouched].tobytes() == clean[:, untouched].tobytes()
    want, bound, l, q = reference(tampered, x)  # the statement clamps as the kernels do
    assert np.isfinite(got).all() and (np.abs(got.astype(np.float64) - want) <= bound).all()
    # posteriors: frame_state far above M - 1 counts as M - 1, any negative value as -1; the tampered comp_off on top
    fs = rng.randint(0, M, frames).astype(np.int32)
    fs_bad = fs.copy()
    fs_bad[[3, 17, 40, 41]] = [M, 1 << 30, -(1 << 30), -7]
    xg = Guarded(x.size).set(x)
    out = {}
    for name, mdl, f in (("clean", model, fs), ("fs", model, fs_bad), ("both", tampered, fs_bad)):
        gamma = Guarded(frames * 8)
        with launched(GPOST):
            A.launch_gmm_post(mdl.views, xg.t, torch.from_numpy(f).to(DEV), gamma.t, frames)
        assert gamma.intact() and xg.intact() and mdl.intact()
        out[name] = gamma.np().reshape(frames, 8)
    same = np.setdiff1d(np.arange(frames), [3, 17, 40, 41])
    assert out["fs"][same].tobytes() == out["clean"][same].tobytes() and not out["fs"][[40, 41]].any()
    for f in (3, 17):
        assert np.allclose(out["fs"][f], G.posteriors(G.comp_loglik(x[f : f + 1], *params)[0], comp_off, [M - 1])[0][0], rtol=1e-3, atol=1e-6)
    keep = same[np.isin(fs[same], untouched)]
    assert len(keep) > 20 and out["both"][keep].tobytes() == out["clean"][keep].tobytes()
    assert np.isfinite(out["both"]).all() and (np.abs(out["both"][fs_bad >= 0].sum(axis=1) - 1.0) <= 10 * U).all()
    # statistics: one row per state over a few frames; wild row tables for some states, the tampered comp_off for others
    row_state = np.arange(M, dtype=np.int32)
    mp = A.AlignMaps([frames], [(row_state, np.zeros(M, np.int32))], M, DEV)
    row_begin, row_frames = (np.arange(M) % (frames - 4)).astype(np.int32), np.full(M, 3, np.int32)
    gam = rng.uniform(0.0, 1.0, (frames, 8)).astype(np.float32)
    gg = Guarded(gam.size).set(gam)

    def stats(off, rb, rf, tamper=None):
        acc = [Guarded(Gn, torch.float64).set(np.zeros(Gn)), Guarded(Gn * D, torch.float64).set(np.zeros(Gn * D)), Guarded(Gn * D, torch.float64).set(np.zeros(Gn * D))]
        og = Guarded(M + 1, torch.int32).set(off)
        maps = A.AlignMaps([frames], [(row_state, np.zeros(M, np.int32))], M, DEV)
        if tamper is not None:
            tamper(maps)
        with launched(GSTATS):
            A.launch_gmm_stats(maps, og.t, xg.t, gg.t, torch.from_numpy(rb).to(DEV), torch.from_numpy(rf).to(DEV), acc[0].t, acc[1].t.view(Gn, D), acc[2].t.view(Gn, D))
        assert all(a.intact() for a in acc) and og.intact() and gg.intact() and xg.intact()
        return [a.np() for a in acc]

    base = stats(comp_off, row_begin, row_frames)
    want = [np.zeros(Gn), np.zeros((Gn, D)), np.zeros((Gn, D))]
    G.stats_chain(x, gam, row_begin, row_frames, mp.state_offs, mp.state_rows_h, comp_off, *want)
    assert all(a.tobytes() == w.tobytes() for a, w in zip(base, want))
    rb, rf = row_begin.copy(), row_frames.copy()
    rb[100:105], rf[105:110] = [1 << 30, -(1 << 30), frames, frames - 1, -1], [1 << 30, -3, frames, 1 << 20, 0]

    def wild_lists(maps):
        off, rows = maps.state_offs.copy(), maps.state_rows_h.copy()
        off[120:125] = [1 << 30, -(1 << 30), 5, 1 << 20, -1]
        rows[130:135] = [1 << 30, -(1 << 30), M, -1, 1 << 20]
        maps.state_off, maps.state_rows = torch.from_numpy(off.astype(np.int32)).to(DEV), torch.from_numpy(rows.astype(np.int32)).to(DEV)

    got = stats(bad, rb, rf, tamper=wild_lists)
    g0, cnt = G.state_comps(bad, Gn)
    hit = np.zeros(Gn, dtype=bool)  # the components a tampered state may have written
    for m in np.setdiff1d(np.arange(M), untouched).tolist() + list(range(100, 110)) + list(range(119, 136)):
        hit[g0[m] : g0[m] + cnt[m]] = True
        hit[comp_off[m] : comp_off[m + 1]] = True
    assert 200 < (~hit).sum() < Gn and all(np.isfinite(a).all() for a in got)
    for a, b in zip(got, base):
        assert a.reshape(Gn, -1)[~hit].tobytes() == b.reshape(Gn, -1)[~hit].tobytes()


def test_refused_inputs_launch_nothing(A):
    from fcl_taco2_amd import _lib

    z = lambda *shape, dt=torch.float32: torch.zeros(*shape, device=DEV, dtype=dt)
    mp = A.AlignMaps([10], [(np.zeros(3, np.int32), np.zeros(3, np.int32))], 4, DEV)
    with launched(absent=(GLOGLIK, GPOST, GSTATS)):
        for Gn, M, D, max_comp in ((36, 4, 4, 9), (8193, 1024, 4, 8), (8, 4, 41, 2)):  # C = 9, G = 8193, D = 41
            params = (z(Gn, D), z(Gn, D), z(Gn), z(M + 1, dt=torch.int32))
            with pytest.raises(_lib.FclError, match="error -2"):
                A.launch_gmm_loglik(params, z(10, D), z(10, M), 10, max_comp)
            with pytest.raises(_lib.FclError, match="error -2"):
                A.launch_gmm_post(params, z(10, D), z(10, dt=torch.int32), z(10, 8), 10, max_comp)
            if M == 4:
                with pytest.raises(_lib.FclError, match="error -2"):
                    A.launch_gmm_stats(mp, params[3], z(10, D), z(10, 8), z(3, dt=torch.int32), z(3, dt=torch.int32), z(Gn, dt=torch.float64),
                                       z(Gn, D, dt=torch.float64), z(Gn, D, dt=torch.float64), max_comp=max_comp)
        params = (z(8, 4), z(8, 4), z(8), z(5, dt=torch.int32))  # an empty batch is no error and no launch
        A.launch_gmm_loglik(params, z(1, 4), z(1, 4), 0, 2)
        A.launch_gmm_post(params, z(1, 4), z(1, dt=torch.int32), z(1, 8), 0, 2)


# ---- fit ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_fit_with_mixtures_reaches_the_float64_trainers_accuracy(A):
    """Aligner.fit on corpus_voices(1): 6 single-Gaussian rounds, then 4 components in 4 + 4 rounds, min_occupancy 10, in two batches.  Demanded: a
    frame accuracy of at least the float64 trainer's on the same corpus less 0.005, and at least the device's own single-Gaussian accuracy plus 0.03.
    Measured on MI355X: see DESIGN 6v."""
    c = G.corpus_voices(1)
    K = c["K"]
    phones = ["p%d" % i for i in range(R.N_PHONES)] + ["sp"]
    transcripts = [[phones[m // K] for m in g[0][::K]] for g in c["graphs"]]
    feats = [torch.from_numpy(x) for x in c["feats"]]
    cells = sum(len(x) * len(g[0]) for x, g in zip(c["feats"], c["graphs"]))
    al = A.Aligner(DEV, phones, K, optional=("sp",), batch_cells=cells // 2 + 1)
    models = {}
    with launched(LOGLIK, VITERBI, STATS, GLOGLIK, GPOST, GSTATS):
        hist = al.fit(feats, transcripts, callback=lambda it, m: models.__setitem__(it, m), **G.SCHEDULE)
        res = al.align(feats, transcripts)
    assert len(hist["score"]) == 14 and hist["failed"] == [[]] * 14 and hist["components"][:10] == [39] * 6 + [78] * 4 and len(set(hist["components"][10:])) == 1
    assert al.model.is_mixture and al.model.max_components == 4 and al.model.n_components == hist["components"][-1] and models[13] is al.model
    assert not models[5].is_mixture and models[6].n_components == 78
    with launched(LOGLIK, absent=(GLOGLIK, GPOST, GSTATS, STATS)):
        res1 = A.Aligner(DEV, model=models[5], optional=("sp",)).align(feats, transcripts)
    acc = R.frame_accuracy([r["row_frames"] for r in res], c["row_phone"], c["truth"])
    single = R.frame_accuracy([r["row_frames"] for r in res1], c["row_phone"], c["truth"])
    ref_single, _, ref, ref_model = G.fit_voices(1)
    print("fit with mixtures: frame accuracy %.4f on the device (%.4f with its single Gaussians, %d components), %.4f in float64 (%.4f, %d components)"
          % (acc, single, al.model.n_components, ref, ref_single, len(ref_model["weight"])))
    assert acc >= ref - 0.005 and acc >= single + 0.03
    for r, x in zip(res, c["feats"]):
        assert r["ok"] and sum(r["durations"]) == len(x)


# ---- driver -------------------------------------------------------------------------------------------------------------------------------------------------
FS, HOP = 22050, 256
TONES = dict(aa=300.0, iy=800.0, uw=1800.0, sh=3500.0)


def _write_wav(path, x, rate=FS):
    pcm = np.clip(np.rint(np.asarray(x, dtype=np.float64) * 32767.0), -32768, 32767).astype("<i2")
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(rate)
        f.writeframes(pcm.tobytes())


@pytest.fixture(scope="module")
def speech(tmp_path_factory):
    """the 8 wavs of test_gpu_align.py's driver test, generated again: one sinusoid per "phoneme", low-level noise for the pause, which the
    transcript has between two phonemes and every other recording leaves out"""
    root = tmp_path_factory.mktemp("align_gmm")
    (root / "wavs").mkdir()
    rng = np.random.RandomState(11)
    names = sorted(TONES)
    lines = []
    for u in range(8):
        labels = [names[i] for i in rng.permutation(4)] + [names[int(rng.randint(4))]]
        labels.insert(2, "sp")
        frames = [0 if p == "sp" and u % 2 else int(rng.randint(5, 10)) for p in labels]
        x = np.concatenate([(0.3 * np.sin(2 * np.pi * TONES[p] * np.arange(n * HOP) / FS) if p != "sp" else np.zeros(n * HOP)) for p, n in zip(labels, frames)])
        x = x[: len(x) - int(rng.randint(1, HOP))]
        x = x + 1e-3 * rng.randn(len(x))
        _write_wav(root / "wavs" / ("utt%d.wav" % u), x)
        lines.append("utt%d " % u + " ".join(labels))
    (root / "phones.txt").write_text("\n".join(lines) + "\n")
    return dict(root=root, ids=[ln.split()[0] for ln in lines], transcripts={ln.split()[0]: ln.split()[1:] for ln in lines})


def test_driver_with_mixtures(A, speech):
    """python -m fcl_taco2_amd.align --mixtures 2 --min-occupancy 2: the TextGrids read back to the durations Aligner.align returns with the saved
    mixtures; --model on them writes byte-identical TextGrids without a statistics launch; the report lists `components` per round; --mixtures 1
    writes the same bytes as no flag"""
    from fcl_taco2_amd import align as drv, extract_features as X, features, textgrid as TG

    root, ids = speech["root"], speech["ids"]
    common = ["--wav-dir", str(root / "wavs"), "--transcripts", str(root / "phones.txt"), "--optional", "sp", "--verbose", "0", "--iterations", "4"]

    def run(tag, extra):
        return drv.main(common + ["--textgrid-out", str(root / ("tg" + tag)), "--durations-out", str(root / ("dur" + tag)), "--model-out", str(root / ("m%s.npz" % tag)),
                                  "--report", str(root / ("rep%s.json" % tag))] + extra)

    with launched(LOGLIK, VITERBI, STATS, GLOGLIK, GPOST, GSTATS):
        doc = run("2", ["--mixtures", "2", "--min-occupancy", "2"])
    assert json.load(open(root / "rep2.json")) == doc and doc["n_aligned"] == 8 and doc["settings"]["mixtures"] == 2 and doc["settings"]["trained"] is True
    comps = [it["components"] for it in doc["iterations"]]
    assert len(comps) == 8 and comps[:4] == [15] * 4 and len(set(comps[4:])) == 1 and 15 < comps[4] <= 30
    model = A.AlignModel.load(str(root / "m2.npz"))
    assert model.is_mixture and model.n_components == comps[-1] and model.max_components == 2 and model.dim == 28
    af = A.AlignFeatures(features.FeatureExtractor(features.FeaturePlan(DEV)))
    feats = af.from_waves([X.read_wav(str(root / "wavs" / (u + ".wav")), FS) for u in ids], ids=ids)
    trs = [speech["transcripts"][u] for u in ids]
    with launched(GLOGLIK, VITERBI, absent=(LOGLIK, STATS, GSTATS)):
        res = A.Aligner(DEV, model=model, optional=("sp",)).align(feats, trs, ids=ids)
    for u, r, x in zip(ids, res, feats):
        assert r["ok"] and sum(r["durations"]) == x.shape[0]
        got_phones, got = TG.alignment(TG.read_textgrid(str(root / "tg2" / (u + ".TextGrid")))["phones"], FS, HOP)
        assert got_phones == r["phones"] and got == r["durations"][:-1] + [r["durations"][-1] - 1]
        assert list(np.load(root / "dur2" / (u + ".npy"))) == r["durations"]
    with launched(GLOGLIK, VITERBI, absent=(LOGLIK, STATS, GSTATS, GPOST)):
        doc2 = drv.main(common + ["--textgrid-out", str(root / "tg2m"), "--model", str(root / "m2.npz"), "--mixtures", "7"])  # the flag is ignored
    assert doc2["iterations"] == [] and doc2["settings"]["trained"] is False and doc2["settings"]["mixtures"] == 2 and doc2["score_per_frame"] == doc["score_per_frame"]
    for u in ids:
        assert (root / "tg2m" / (u + ".TextGrid")).read_bytes() == (root / "tg2" / (u + ".TextGrid")).read_bytes()
    # --mixtures 1 is no flag at all
    with launched(LOGLIK, VITERBI, STATS, absent=(GLOGLIK, GPOST, GSTATS)):
        a, b = run("a", []), run("b", ["--mixtures", "1", "--mix-iterations", "9", "--min-occupancy", "3"])
    assert "mixtures" not in a["settings"] and all("components" not in it for it in a["iterations"]) and len(a["iterations"]) == 4
    assert (root / "repa.json").read_bytes() == (root / "repb.json").read_bytes() and (root / "ma.npz").read_bytes() == (root / "mb.npz").read_bytes()
    for u in ids:
        assert (root / "tga" / (u + ".TextGrid")).read_bytes() == (root / "tgb" / (u + ".TextGrid")).read_bytes()
        assert (root / "dura" / (u + ".npy")).read_bytes() == (root / "durb" / (u + ".npy")).read_bytes()
