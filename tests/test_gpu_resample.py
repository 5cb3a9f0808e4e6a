"""csrc/resample.hip against the float64 numpy statement of tests/resample_ref.py.  The input and the output sit between guard zones
filled with a NaN bit pattern, which must survive (and poison any sum that reads them); every test reads the library's launch record and fails if the
kernel did not run.  The statement itself is checked in test_resample_cpu.py."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import resample_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAT32 = 0x7FC12345  # an fp32 NaN
KERNEL = "rs_resample_kernel"


@pytest.fixture(scope="module")
def RS():
    assert torch.cuda.is_available()
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib, resample

    _lib.load()
    return resample


@contextlib.contextmanager
def launch_record(seen):
    """collects the names of the kernels launched inside into `seen` (the library's own launch record)"""
    from fcl_taco2_amd import _lib

    _lib.prof_enable(True)
    try:
        yield
        torch.cuda.synchronize()
        seen.update(_lib.prof_collect())
    finally:
        _lib.prof_enable(False)


class Guarded(object):
    """a float32 device buffer of n words between two guard zones; everything starts as the NaN pattern"""

    PAD = 8192

    def __init__(self, n):
        self.n = int(n)
        self.buf = torch.empty(self.n + 2 * self.PAD, dtype=torch.float32, device=DEV)
        self.buf.view(torch.int32).fill_(PAT32)

    @property
    def t(self):
        return self.buf[self.PAD : self.PAD + self.n]

    def set(self, a):
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).reshape(-1))
        return self

    def np(self):
        return self.t.cpu().numpy()

    def intact(self):
        b = self.buf.view(torch.int32)
        return bool((b[: self.PAD] == PAT32).all()) and bool((b[self.PAD + self.n :] == PAT32).all())


@functools.lru_cache(maxsize=None)
def reference(pair, lens=None):
    """computed once per rate pair and shared: the utterances (loud noise; the long ones carry an impulse at their first and last sample, so that
    both zero-filled edges carry signal), and per utterance y and sum |c x| in float64"""
    L, M = R.ratio(*pair)
    K = R.half_width(L, M)
    c = R.table(L, M)
    rng = np.random.RandomState(sum(pair))
    lens = [1, 2, K, K + 1, 2 * K + 1, 2 * K + 2, 3001, 4999] if lens is None else list(lens)
    xs = []
    for n in lens:
        x = (0.9 * (2.0 * rng.rand(n) - 1.0)).astype(np.float32)
        if n > 3000:
            x[0], x[-1] = 1.0, -1.0
        x.setflags(write=False)
        xs.append(x)
    per = [R.resample(x.astype(np.float64), L, M, c) for x in xs]
    out_lens = [R.out_samples(n, L, M) for n in lens]
    assert [len(y) for y, _ in per] == out_lens
    return dict(L=L, M=M, K=K, c=c, xs=xs, lens=lens, out_lens=out_lens, per=per)


def run(RS, pl, xs):
    """one launch on guarded buffers -> the output bytes per utterance"""
    lens = [len(x) for x in xs]
    out_lens = [pl.out_samples(n) for n in lens]
    x = Guarded(sum(lens)).set(np.concatenate(xs))
    y = Guarded(sum(out_lens))
    seen = set()
    with launch_record(seen):
        RS.launch_resample(pl, x.t, RS.offsets(lens, DEV), RS.offsets(out_lens, DEV), y.t, len(xs), sum(lens), sum(out_lens), max(out_lens))
    assert KERNEL in seen, sorted(seen)
    assert x.intact() and y.intact()
    off = np.concatenate([[0], np.cumsum(out_lens)])
    got = y.np()
    return [got[off[i] : off[i + 1]] for i in range(len(xs))]


def check_vs_float64(RS, pair, ref):
    """one guarded launch over ref's utterances: every output within the bound of float64; -> the plan and the outputs"""
    pl = RS.ResamplePlan(DEV, *pair)
    assert (pl.L, pl.M, pl.K) == (ref["L"], ref["M"], ref["K"]) and pl.table.shape == ref["c"].shape and np.abs(pl.table - ref["c"]).max() <= 1e-14
    assert np.array_equal(pl.table_d.cpu().numpy(), pl.table.T.astype(np.float32))
    assert [pl.out_samples(n) for n in ref["lens"]] == ref["out_lens"]
    got = run(RS, pl, ref["xs"])
    worst, n_checked = 0.0, 0
    for g, (y64, a) in zip(got, ref["per"]):
        assert g.shape == y64.shape and np.isfinite(g).all()
        if len(g):
            assert (a > 0).all()
            worst = max(worst, float((np.abs(g.astype(np.float64) - y64) / R.bound(a, ref["K"])).max()))
            n_checked += len(g)
    print("resample %r: L / M = %d / %d, K = %d, %d outputs, worst share of the bound %.3f" % (pair, ref["L"], ref["M"], ref["K"], n_checked, worst))
    assert worst <= 1.0 and n_checked == sum(ref["out_lens"])
    return pl, got


@pytest.mark.parametrize("pair", R.PAIRS, ids=str)
def test_resampled_batch_vs_float64(RS, pair):
    """Eight packed utterances (shorter than the filter, n_out = 0 when downsampling 1 or 2 samples, several tiles with a partial last one): for every
    output |y - y64| <= (2 K + 3) 2^-24 sum_j |c[p][j] x[n - j]|, the running bound of a float32 fma chain on float32-rounded coefficients."""
    ref = reference(pair)
    _, got = check_vs_float64(RS, pair, ref)
    if ref["M"] > ref["L"]:
        assert ref["out_lens"][:2] == [0, 2 * ref["L"] // ref["M"]] and len(got[0]) == 0  # an utterance without output inside the batch


def test_outputs_in_order_where_a_period_does_not_fit_the_tile(RS):
    """8100 Hz -> 199 Hz (L / M = 199 / 8100, K = 2606, a 4.1 MB table): the 5213-tap span leaves room for a tile of 174 outputs, fewer than the 199 of a
    period, so the threads take the outputs in order instead of by phase.  Three tiles, the last partial; the same bound; batch = single runs."""
    pair = (8100, 199)
    ref = reference(pair, (2606, 5214, 20000))
    assert (ref["L"], ref["M"], ref["K"]) == (199, 8100, 2606) and ref["out_lens"] == [64, 128, 491]
    pl, got = check_vs_float64(RS, pair, ref)
    for i, x in enumerate(ref["xs"]):
        assert run(RS, pl, [x])[0].tobytes() == got[i].tobytes(), i


@pytest.mark.parametrize("pair", R.PAIRS, ids=str)
def test_batch_equals_per_utterance_runs_bit_for_bit(RS, pair):
    """one launch over the eight utterances against one launch each (other tiles, other neighbours: the same bits), and the public entry"""
    ref = reference(pair)
    pl = RS.ResamplePlan(DEV, *pair)
    got = run(RS, pl, ref["xs"])
    for i, x in enumerate(ref["xs"]):
        if ref["out_lens"][i]:
            assert run(RS, pl, [x])[0].tobytes() == got[i].tobytes(), i
    rs = RS.Resampler(pl)
    seen = set()
    with launch_record(seen):
        y, out_lens = rs.resample_packed(np.concatenate(ref["xs"]), ref["lens"])
        y1, l1 = rs.resample_packed(np.array(ref["xs"][0]), [1])  # downsampling: no output, no launch
    assert KERNEL in seen and out_lens == ref["out_lens"] and y.cpu().numpy().tobytes() == np.concatenate(got).tobytes()
    assert l1 == [ref["out_lens"][0]] and y1.numel() == l1[0]
    with pytest.raises(RS._lib.FclError, match="lens sum to 7"):
        rs.resample_packed(np.array(ref["xs"][-1]), [7])


def test_identity_and_refused_rates(RS):
    """equal rates: the samples come back and nothing is launched; L > 1024 is refused naming both rates"""
    x = np.array(reference((16000, 22050))["xs"][-1])
    pl = RS.ResamplePlan(DEV, 22050, 22050)
    assert pl.identity and pl.table is None
    seen = set()
    with launch_record(seen):
        y, lens = RS.Resampler(pl).resample_packed(x, [len(x)])
    assert KERNEL not in seen and lens == [len(x)] and np.array_equal(y.cpu().numpy(), x)
    with pytest.raises(NotImplementedError, match="22050 Hz -> 22051 Hz"):
        RS.ResamplePlan(DEV, 22050, 22051)
