"""-m gpu: fcl_variance_embed_rows_fwd against the two launches it replaces -- fcl_variance_embed_add[_ctl]_fwd followed by fcl_gather_rows_fwd(planes) --
on the same inputs, BIT FOR BIT in both planes (the int16 plane buffers are compared as they are), with NaN-pattern guard lines in front of and behind
the output.  Shapes: C = 256 (one channel group per wave), 32 (a wave with 8 working lanes), 288 (two channel groups); k = 9 (the unrolled
instantiation), 3 and 1 (the general one); m = 1, 17, 130 source rows in one to four segments, with segments of length 1 and 2 (shorter than the window)
and a boundary inside the window of the first and of the last row; 0, 1, 5 and 130 destination rows (5 and 130 are no multiples of the 4 rows a wave
walks), permuted, repeated, some -1."""
import numpy as np
import pytest
import torch

from fcl_taco2_amd import _lib, plan as PL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 2  # rows of guard lines on either side
PATTERN = 0x7FC1  # a bf16 NaN in both planes

SEGS = {1: [[1]], 17: [[17], [3, 14], [15, 2], [1, 2, 9, 5]], 130: [[130], [3, 127], [1, 2, 64, 63], [100, 28, 2]]}


@pytest.fixture(scope="module")
def ops():
    from fcl_taco2_amd import ops as o

    return o


def _segments(lens):
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    lo = np.concatenate([np.full(n, s, np.int32) for n, s in zip(lens, starts)])
    hi = np.concatenate([np.full(n, s + n, np.int32) for n, s in zip(lens, starts)])
    return lo, hi


def _inputs(rng, m, c, k):
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    f = lambda *s: d(rng.standard_normal(s).astype(np.float32))
    return dict(hs=f(m, c), p=f(m), e=f(m), wp=f(c, k), bp=f(c), we=f(c, k), be=f(c))


def _src_rows(rng, m, n):
    src = np.concatenate([rng.permutation(m), rng.randint(0, m, max(n - m, 0))])[:n].astype(np.int32)
    if n >= 5:
        src[rng.choice(n, n // 4, replace=False)] = -1
    return torch.from_numpy(src).to(DEV)


def _fused(ops, x, lo, hi, src, ctl=None, row_div=1, scalars=False):
    """The new entry, called directly so that the output sits between guard lines.  Returns (planes [n, C / 32 * 64] int16, p_out, e_out)."""
    m, c = x["hs"].shape
    n, k, w = src.numel(), x["wp"].shape[1], c // 32 * 64
    buf = torch.full((n + 2 * GUARD, w), PATTERN, device=DEV, dtype=torch.int16)
    p_out = torch.full_like(x["p"], float("nan")) if scalars else None
    e_out = torch.full_like(x["e"], float("nan")) if scalars else None
    ptr = lambda t: None if t is None else t.data_ptr()
    wpt, wet = PL.tap_major(x["wp"]), PL.tap_major(x["we"])
    rc = _lib.load().fcl_variance_embed_rows_fwd(ptr(x["hs"]), ptr(x["p"]), ptr(x["e"]), ptr(wpt), ptr(x["bp"]), ptr(wet), ptr(x["be"]), ptr(lo), ptr(hi), ptr(src),
                                                 ptr(ctl), 0 if ctl is None else ctl.shape[1], row_div, buf.data_ptr() + GUARD * w * 2, ptr(p_out), ptr(e_out),
                                                 m, n, c, k, torch.cuda.current_stream().cuda_stream)
    _lib.check(rc)
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == PATTERN).all()) and bool((buf[GUARD + n:] == PATTERN).all()), "guard lines overwritten"
    return buf[GUARD:GUARD + n], p_out, e_out


def _two_launches(ops, x, lo, hi, src, ctl=None, row_div=1):
    if ctl is None:
        att, _, _ = ops.variance_embed_add(x["hs"], x["p"], x["e"], x["wp"], x["bp"], x["we"], x["be"], lo, hi)
        p_out = e_out = None
    else:
        att, _, _, p_out, e_out = ops.variance_embed_add_ctl(x["hs"], x["p"], x["e"], x["wp"], x["bp"], x["we"], x["be"], lo, hi, ctl, row_div)
    n = src.numel()
    planes = ops.gather_rows(att, src, want_f32=False, want_planes=True)[1][:n] if n else None
    return planes, p_out, e_out


@pytest.mark.parametrize("k", [9, 3, 1])
@pytest.mark.parametrize("c", [256, 32, 288])
def test_rows_equal_embed_then_gather_bit_for_bit(ops, c, k):
    rng = np.random.RandomState(1000 * c + k)
    for m in (1, 17, 130):
        x = _inputs(rng, m, c, k)
        for lens in SEGS[m]:
            lo, hi = (torch.from_numpy(a).to(DEV) for a in _segments(lens))
            for n in (0, 1, 5, 130):
                src = _src_rows(rng, m, n)
                got, _, _ = _fused(ops, x, lo, hi, src)
                ref, _, _ = _two_launches(ops, x, lo, hi, src)
                if n:
                    assert torch.equal(got, ref), (m, lens, n)
                    dead = (src < 0).nonzero().flatten()
                    assert not bool(got[dead].any())  # an index of -1: zeros in both planes


@pytest.mark.parametrize("k", [9, 3])
@pytest.mark.parametrize("c", [256, 32, 288])
def test_controlled_form_equals_the_controlled_launches_bit_for_bit(ops, c, k):
    rng = np.random.RandomState(7000 * c + k)
    for m, div in ((17, 1), (130, 1), (130, 26)):  # one control per row; one per utterance of a padded [5, 26] layout (ctl_row_div = T)
        x = _inputs(rng, m, c, k)
        rows = (m - 1) // div + 1
        ident = np.tile(np.array([1, 1, 0, 1, 0], np.float32), (rows, 1))
        mixed = ident.copy()
        mixed[:, 1] = rng.choice([1.0, 1.3, 0.7], rows)
        mixed[:, 2] = rng.choice([0.0, 0.25, -0.5], rows)
        mixed[:, 3] = rng.choice([1.0, 0.9, 1.6], rows)
        mixed[:, 4] = rng.choice([0.0, 0.1], rows)
        mixed[0, 1:] = [1.2, 0.3, 0.8, -0.2]  # at least one row with every control away from identity
        for lens in SEGS[m][1:]:
            lo, hi = (torch.from_numpy(a).to(DEV) for a in _segments(lens))
            for n in (5, 130):
                src = _src_rows(rng, m, n)
                plain, _, _ = _fused(ops, x, lo, hi, src)
                for name, c_np in (("identity", ident), ("mixed", mixed)):
                    ctl = torch.from_numpy(c_np).to(DEV)
                    got, p_out, e_out = _fused(ops, x, lo, hi, src, ctl, div, scalars=True)
                    ref, p_ref, e_ref = _two_launches(ops, x, lo, hi, src, ctl, div)
                    assert torch.equal(got, ref), (name, m, div, lens, n)
                    assert torch.equal(p_out, p_ref) and torch.equal(e_out, e_ref), (name, m, div)
                    if name == "identity":  # identity controls: the plain form, bit for bit, and the predictions untouched
                        assert torch.equal(got, plain) and torch.equal(p_out, x["p"]) and torch.equal(e_out, x["e"])
                    elif n == 130:  # (every source row is among the destinations: the controls of row 0 are felt)
                        assert not torch.equal(got, plain)


def test_scalars_only_and_the_wrapper(ops):
    """n == 0 with p_out / e_out: only the controlled scalars are written; ops.variance_embed_rows returns what the direct call does; bad shapes are refused."""
    rng = np.random.RandomState(5)
    m, c, k = 130, 256, 9
    x = _inputs(rng, m, c, k)
    lo, hi = (torch.from_numpy(a).to(DEV) for a in _segments([100, 28, 2]))
    ctl = torch.from_numpy(np.tile(np.array([1, 1.1, 0.2, 0.9, -0.1], np.float32), (m, 1))).to(DEV)
    _, p_out, e_out = _fused(ops, x, lo, hi, _src_rows(rng, m, 0), ctl, 1, scalars=True)
    _, p_ref, e_ref = _two_launches(ops, x, lo, hi, _src_rows(rng, m, 0), ctl, 1)
    assert torch.equal(p_out, p_ref) and torch.equal(e_out, e_ref)
    src = _src_rows(rng, m, 77)
    planes, p2, e2 = ops.variance_embed_rows(x["hs"], x["p"], x["e"], PL.tap_major(x["wp"]), x["bp"], PL.tap_major(x["we"]), x["be"], lo, hi, src, ctl, 1,
                                            want_scalars=True)
    torch.cuda.synchronize()
    assert torch.equal(planes, _fused(ops, x, lo, hi, src, ctl, 1)[0]) and torch.equal(p2, p_ref) and torch.equal(e2, e_ref)
    lib = _lib.load()
    z = x["hs"].data_ptr()
    assert lib.fcl_variance_embed_rows_fwd(z, z, z, z, z, z, z, z, z, z, None, 0, 1, z, None, None, 4, 4, 36, 9, None) == -2 and b"multiple of 32" in lib.fcl_last_error()
    assert lib.fcl_variance_embed_rows_fwd(z, z, z, z, z, z, z, z, z, z, None, 0, 1, z, None, None, 4, 4, 32, 4, None) == -1  # even k
    assert lib.fcl_variance_embed_rows_fwd(z, z, z, z, z, z, z, z, z, None, None, 0, 1, None, None, None, 4, 4, 32, 3, None) == -1  # rows without src_rows / out_p
