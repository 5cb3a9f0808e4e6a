"""CPU-only: the row semantics of fcl_variance_embed_rows_fwd restated in numpy (rows_ref) and checked against torch float64 conv1d + add + index on
the small shapes the GPU test uses; the tap-major weight table of the plan is the exact transpose of the Conv1d weights.

rows_ref is the contract of the kernel: destination row i is row r = src_rows[i] of (hs + p_emb) + e_emb, an index outside [0, m) gives a zero row, a tap
j is admitted when seg_lo[r] <= r + j - pad < seg_hi[r], and the admitted taps are taken in order j = 0 .. k - 1 with a fused multiply-add.

Tolerance.  Per channel the fp32 result is a chain of at most k fused multiply-adds on the bias (one rounding each), twice, and two additions: 2 k + 2
roundings, each at most half an ulp of an intermediate whose magnitude is bounded by S = |hs| + |bp| + |be| + sum_j |wp_j p_j| + sum_j |we_j e_j|.  The
float64 reference adds its own (negligible) error.  So |fp32 - float64| <= (2 k + 2) * eps32 * S, i.e. within one ulp (2 * the half-ulp bound) per tap."""
import numpy as np
import pytest
import torch

from fcl_taco2_amd import plan as PL

EPS32 = float(np.finfo(np.float32).eps)


def fma32(a, b, c):
    """fmaf on float32 arrays: the product of two float32 is exact in float64; one rounding to float32 at the end (the float64 addition's own rounding
    changes the result only in double-rounding corner cases, far below the tolerance of this file)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def rows_ref(hs, p, e, wp, bp, we, be, seg_lo, seg_hi, src_rows):
    """numpy restatement, float32 arithmetic in the kernel's order.  wp / we: [C, k]."""
    m, c = hs.shape
    k = wp.shape[1]
    pad = (k - 1) // 2
    out = np.zeros((len(src_rows), c), np.float32)
    for i, r in enumerate(src_rows):
        if r < 0 or r >= m:
            continue  # zero row
        ap, ae = bp.copy(), be.copy()
        for j in range(k):
            q = r + j - pad
            if seg_lo[r] <= q < seg_hi[r]:
                ap = fma32(wp[:, j], np.full(c, p[q], np.float32), ap)
                ae = fma32(we[:, j], np.full(c, e[q], np.float32), ae)
        out[i] = (hs[r] + ap) + ae
    return out


def segments(lens):
    lo = np.concatenate([np.full(n, s, np.int32) for n, s in zip(lens, np.concatenate([[0], np.cumsum(lens)[:-1]]))])
    hi = np.concatenate([np.full(n, s + n, np.int32) for n, s in zip(lens, np.concatenate([[0], np.cumsum(lens)[:-1]]))])
    return lo, hi


def rows_f64(hs, p, e, wp, bp, we, be, lens, src_rows):
    """torch float64: Conv1d(1, C, k, padding=(k - 1) // 2) per segment (zero padding at the segment's ends), add, index; plus the magnitude bound S."""
    k = wp.shape[1]
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    outs, mags = [], []
    s = 0
    for n in lens:
        sl = slice(s, s + n)
        conv = lambda x, w, b: torch.nn.functional.conv1d(t(x[sl]).view(1, 1, -1), t(w).view(-1, 1, k), t(b), padding=(k - 1) // 2)[0].t()
        mag = lambda x, w, b: torch.nn.functional.conv1d(t(np.abs(x[sl])).view(1, 1, -1), t(np.abs(w)).view(-1, 1, k), t(np.abs(b)), padding=(k - 1) // 2)[0].t()
        outs.append((t(hs[sl]) + conv(p, wp, bp)) + conv(e, we, be))
        mags.append(t(np.abs(hs[sl])) + mag(p, wp, bp) + mag(e, we, be))
        s += n
    full, S = torch.cat(outs).numpy(), torch.cat(mags).numpy()
    m = full.shape[0]
    ok = np.array([0 <= r < m for r in src_rows], bool)
    idx = np.where(ok, src_rows, 0)
    return np.where(ok[:, None], full[idx], 0.0), np.where(ok[:, None], S[idx], 0.0)


CASES = [(1, [1]), (17, [17]), (17, [3, 14]), (17, [15, 2]), (17, [1, 2, 9, 5]), (130, [130]), (130, [1, 2, 64, 63]), (130, [100, 28, 2])]


@pytest.mark.parametrize("c", [256, 32, 288])
@pytest.mark.parametrize("k", [9, 3, 1])
def test_row_semantics_against_float64_conv1d(c, k):
    rng = np.random.RandomState(100 * c + k)
    for m, lens in CASES:
        hs = rng.standard_normal((m, c)).astype(np.float32)
        p, e = rng.standard_normal(m).astype(np.float32), rng.standard_normal(m).astype(np.float32)
        wp, we = rng.standard_normal((c, k)).astype(np.float32), rng.standard_normal((c, k)).astype(np.float32)
        bp, be = rng.standard_normal(c).astype(np.float32), rng.standard_normal(c).astype(np.float32)
        lo, hi = segments(lens)
        for n in (0, 1, 5, 130):
            src = rng.randint(0, m, n).astype(np.int32)
            if n >= 5:
                src[rng.choice(n, n // 4 + 1, replace=False)] = -1
                src[-1] = m  # past the end: a zero row as well
            got = rows_ref(hs, p, e, wp, bp, we, be, lo, hi, src)
            ref, S = rows_f64(hs, p, e, wp, bp, we, be, lens, src)
            assert got.shape == (n, c)
            assert (np.abs(got - ref) <= (2 * k + 2) * EPS32 * S).all(), (m, lens, n, float(np.abs(got - ref).max()))
            assert not got[(src < 0) | (src >= m)].any()


def test_admission_and_tap_order_on_a_hand_case():
    # one channel, k = 3, two segments [0, 2) and [2, 3): row 1 admits taps 0 and 1 only, row 2 admits tap 1 only
    hs = np.zeros((3, 1), np.float32)
    p, e = np.array([1.0, 2.0, 4.0], np.float32), np.zeros(3, np.float32)
    wp, we = np.array([[1.0, 10.0, 100.0]], np.float32), np.zeros((1, 3), np.float32)
    z = np.zeros(1, np.float32)
    lo, hi = segments([2, 1])
    out = rows_ref(hs, p, e, wp, z, we, z, lo, hi, np.array([2, 1, -1, 0], np.int32))
    assert out[:, 0].tolist() == [40.0, 1.0 * 1 + 10.0 * 2, 0.0, 10.0 * 1 + 100.0 * 2]
    # the order of the taps matters in fp32: 1e8 + 1 - 1e8 taken left to right loses the 1
    p = np.array([1e8, 1.0, -1e8], np.float32)
    out = rows_ref(hs, p, e, np.ones((1, 3), np.float32), z, we, z, *segments([3]), np.array([1], np.int32))
    assert out[0, 0] == 0.0


def test_tap_major_table_is_the_exact_transpose():
    rng = np.random.RandomState(3)
    for c, k in ((256, 9), (32, 3), (288, 1)):
        w = rng.standard_normal((c, 1, k)).astype(np.float32)  # Conv1d(1, C, k).weight
        t = PL.tap_major(w)
        assert t.shape == (k, c) and t.flags["C_CONTIGUOUS"] and np.array_equal(t, w[:, 0, :].T)
        tt = PL.tap_major(torch.from_numpy(w).reshape(c, k))
        assert tt.is_contiguous() and tt.shape == (k, c) and np.array_equal(tt.numpy(), w[:, 0, :].T)
