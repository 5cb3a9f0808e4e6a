"""float64 statement of the synthesis encoder's first stage as a table lookup (include/fcl_hip.h fcl_embed_conv_table_fwd): embedding -> Conv1d with
the eval-mode BatchNorm folded in -> activation (-> + the embedding row, `use_residual`), its per-element error bound, a float32 evaluation in the
kernel's order of operations, wrong restatements the bound must reject, and the seeded cases of the tests built on them
(tests/test_embed_conv_table_cpu.py without a GPU, tests/test_gpu_embed_conv_table.py on one).  Plain numpy; nothing here calls, or is derived from, a
kernel of the library.

The statement.  Inputs are the float32 arrays the plan holds: the folded weight wfold [Cout, Cin, k] (W * gamma / sqrt(var + eps)), the folded bias
[Cout] (beta - mean * scale), the embedding table E [V, Cin], and per row r an id and a segment [seg_lo[r], seg_hi[r]) (its utterance's rows).  With
    T[tap][v][co] = sum_ci wfold[co, ci, tap] * E[v, ci]                                                   (float64)
    y[r] = act(bias + sum over tap = 0 .. k-1 of T[tap][ids[r + tap - k/2]] where seg_lo[r] <= r + tap - k/2 < seg_hi[r]) (+ E[ids[r]])
which is Conv1d(padding = k/2) over each utterance on its own, because a row of the convolution's input IS a row of E.  An id outside [0, V) stands
for a zero embedding row (fcl_embedding_fwd's contract): it contributes nothing, to the sum and to the residual.

The bound counts float32 roundings against that float64 value.  As in tests/train_pointwise_ref.py one rounding is counted as one ulp, 2 u = 2^-23
relative (u = 2^-24): a round-to-nearest operation errs by at most half of that, which is why a correct float32 evaluation must stay inside HALF
of the bound (tests/test_embed_conv_table_cpu.py).
  * one rounding per table entry (the tables are accumulated in float64 and rounded ONCE):          2 u * sum_admitted |T|
  * k additions onto the running sum, whose magnitude never exceeds S = |bias| + sum_admitted |T|:   k * 2 u * S
  * ReLU and the identity are exact and 1-Lipschitz; tanh / sigmoid add FLOOR = 1e-6 (the project's floor of one gate-function evaluation);
  * one more addition when the residual is on:                                                       2 u * (|act(.)| + |E[id]|)
times (1 + 2^-16) for the products of at most k + 2 relative errors of 2^-24 each (second order)."""
import zlib

import numpy as np

U = 2.0 ** -24
FLOOR = 1e-6
ACT_NONE, ACT_RELU, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3
BN_EPS = 1e-5
f32 = np.float32


def f64(x):
    return np.asarray(x, dtype=np.float64)


def rng_of(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def act_f64(v, act):
    if act == ACT_RELU:
        return np.maximum(v, 0.0)
    if act == ACT_TANH:
        return np.tanh(v)
    if act == ACT_SIGMOID:
        return 1.0 / (1.0 + np.exp(-v))
    return v


def fold_bn_f64(w, gamma, beta, mean, var, eps=BN_EPS):
    """Conv1d(no bias) + eval BatchNorm as one convolution: (w * scale[co], shift) in float64."""
    scale = f64(gamma) / np.sqrt(f64(var) + eps)
    return f64(w) * scale[:, None, None], f64(beta) - f64(mean) * scale


def tables_f64(wfold, embed):
    """wfold [Cout, Cin, k], embed [V, Cin] -> T [k, V, Cout] float64."""
    return np.einsum("oct,vc->tvo", f64(wfold), f64(embed))


def segments(lens, rows=None):
    """Utterances back to back: (seg_lo, seg_hi) int32 [rows]; rows past the total (rows > sum(lens)) carry an empty segment at the total."""
    total = int(np.sum(lens))
    rows = total if rows is None else rows
    lo, hi = np.full(rows, total, dtype=np.int32), np.full(rows, total, dtype=np.int32)
    s = 0
    for n in lens:
        lo[s : s + n], hi[s : s + n] = s, s + n
        s += n
    return lo, hi


def _taps(tables, ids, seg_lo, seg_hi, lo_shift=0, hi_shift=0):
    """Per tap: (admitted [m] bool, table rows [m, Cout] float64, zero where not admitted)."""
    k, v, cout = tables.shape
    m, pad = ids.shape[0], (k - 1) // 2
    rows = np.arange(m)
    out = []
    for tap in range(k):
        r = rows + tap - pad
        ok = (r >= seg_lo + lo_shift) & (r < seg_hi + hi_shift) & (r >= 0) & (r < m)
        idr = ids[np.clip(r, 0, m - 1)]
        ok &= (idr >= 0) & (idr < v)
        t = np.where(ok[:, None], tables[tap][np.clip(idr, 0, v - 1)], 0.0)
        out.append((ok, t))
    return out


def _residual(embed, ids):
    v = embed.shape[0]
    ok = (ids >= 0) & (ids < v)
    return np.where(ok[:, None], f64(embed)[np.clip(ids, 0, v - 1)], 0.0)


def ref_embed_conv(tables, bias, ids, seg_lo, seg_hi, act, embed=None):
    """The statement above in float64 (tables: tables_f64's float64 result)."""
    acc = np.broadcast_to(f64(bias), (ids.shape[0], tables.shape[2])).copy()
    for _, t in _taps(f64(tables), ids, seg_lo, seg_hi):
        acc = acc + t
    y = act_f64(acc, act)
    return y + _residual(embed, ids) if embed is not None else y


def bound_embed_conv(tables, bias, ids, seg_lo, seg_hi, act, embed=None):
    k = tables.shape[0]
    st = np.zeros((ids.shape[0], tables.shape[2]))
    pre = np.broadcast_to(f64(bias), st.shape).copy()
    for _, t in _taps(f64(tables), ids, seg_lo, seg_hi):
        st += np.abs(t)
        pre += t
    b = 2 * U * st + k * 2 * U * (np.abs(f64(bias))[None, :] + st)
    if act in (ACT_TANH, ACT_SIGMOID):
        b = b + FLOOR
    if embed is not None:
        b = b + 2 * U * (np.abs(act_f64(pre, act)) + np.abs(_residual(embed, ids)))
    return b * (1.0 + 2.0 ** -16)


def f32_embed_conv(tables, bias, ids, seg_lo, seg_hi, act, embed=None):
    """The kernel's order in float32 numpy: tables rounded once, acc = bias, the admitted taps added in order 0 .. k-1, activation, residual."""
    t32 = f64(tables).astype(f32)
    acc = np.broadcast_to(np.asarray(bias, dtype=f32), (ids.shape[0], t32.shape[2])).copy()
    for ok, t in _taps(t32, ids, seg_lo, seg_hi):
        acc = np.where(ok[:, None], (acc + t.astype(f32)).astype(f32), acc)
    if act == ACT_RELU:
        acc = np.maximum(acc, f32(0))
    elif act != ACT_NONE:
        acc = act_f64(f64(acc), act).astype(f32)
    if embed is not None:
        acc = (acc + _residual(embed, ids).astype(f32)).astype(f32)
    return acc


# ---- wrong restatements: each must leave the bound somewhere -------------------------------------------------------------------------------------
def wrong_restatements(tables, bias, ids, seg_lo, seg_hi, act, embed):
    """{name: float64 [m, Cout]} of the statement with one mistake each (embed given: the residual variants apply)."""
    tables, k, v, cout = f64(tables), tables.shape[0], tables.shape[1], tables.shape[2]
    b = np.broadcast_to(f64(bias), (ids.shape[0], cout))
    res = _residual(embed, ids)
    fin = lambda pre: act_f64(pre, act) + res
    sum_of = lambda taps: sum(t for _, t in taps)
    out = {
        "tap order reversed": fin(b + sum_of(_taps(tables[::-1], ids, seg_lo, seg_hi))),
        "segment start one row early": fin(b + sum_of(_taps(tables, ids, seg_lo, seg_hi, lo_shift=-1))),
        "segment start one row late": fin(b + sum_of(_taps(tables, ids, seg_lo, seg_hi, lo_shift=1))),
        "segment end one row early": fin(b + sum_of(_taps(tables, ids, seg_lo, seg_hi, hi_shift=-1))),
        "segment end one row late": fin(b + sum_of(_taps(tables, ids, seg_lo, seg_hi, hi_shift=1))),
        "residual before the activation": act_f64(b + sum_of(_taps(tables, ids, seg_lo, seg_hi)) + res, act),
        "bias dropped": fin(sum_of(_taps(tables, ids, seg_lo, seg_hi))),
        "table read as [co][v]": fin(b + sum_of(_taps(np.stack([tables[t].reshape(cout, v).T for t in range(k)]), ids, seg_lo, seg_hi))),
    }
    return out


# ---- seeded cases ------------------------------------------------------------------------------------------------------------------------------------
SHAPES = [(cout, v, k) for cout in (256, 32) for v in (80, 3) for k in (5, 3)]
ROW_SETS = {"one_row": (1,), "shorter_than_kernel": (1, 2), "boundary_in_group": (5, 12), "three_utts": (40, 57, 33)}


def make_case(cout, v, k, lens, residual, act=ACT_RELU):
    """float32 inputs as the plan holds them + the int arrays of one batch.  Cin = Cout when the residual is on (it adds an embedding row)."""
    rng = rng_of("embed_conv", cout, v, k, tuple(lens), residual, act)
    cin = cout if residual else 20
    w = rng.standard_normal((cout, cin, k)) / np.sqrt(cin * k)
    gamma, beta = 1.0 + 0.3 * rng.standard_normal(cout), 0.2 * rng.standard_normal(cout)
    mean, var = 0.1 * rng.standard_normal(cout), 0.5 + rng.random_sample(cout)
    wf, bf = fold_bn_f64(w, gamma, beta, mean, var)
    embed = rng.standard_normal((v, cin)).astype(f32)
    m = int(np.sum(lens))
    ids = rng.randint(0, v, size=m).astype(np.int64)
    if m == 1:
        ids[0] = 0 if residual else v - 1
    else:
        ids[0], ids[-1] = 0, v - 1
    lo, hi = segments(lens)
    return dict(w=w, bn=(gamma, beta, mean, var), wfold=wf.astype(f32), bias=bf.astype(f32), embed=embed, ids=ids, seg_lo=lo, seg_hi=hi, act=act,
                lens=tuple(lens), residual=residual, cout=cout, cin=cin, v=v, k=k, m=m)
