"""float64 statements of the element-wise and reduction operations of the training step (train-mode BatchNorm statistics / forward / backward, the
activation maps, column sums, the one-input-channel convolution's weight gradient, the tap-major gradient unpack, the speaker concat, channel
LayerNorm forward / backward with dropout, scalar head and pad mask), their per-element error bounds, and the seeded inputs of the tests built on
them (tests/test_train_pointwise_ref_cpu.py without a GPU, tests/test_gpu_train_pointwise_f64.py on one).  Plain numpy; nothing here calls, or is
derived from, a kernel of the library: every ref_* is the operation's definition evaluated in float64 on the float32 inputs the kernel receives
(a `float` argument -- eps, momentum, keep_scale -- enters as the float32 it is passed as: wide()).

Bounds count float32 roundings, u = 2^-24 (a bound of 0 = the element is a copy or a masked zero and must match exactly):
  bn_stats   mean: the float64 sum / M rounded once: 2^-23 |mu| + 1e-12 mean|z|.  invstd = 1 / sqrt(biased var + eps): 2^-23 relative.
             running r' = (1 - m) r + m stat (variance unbiased, var M / (M - 1); var itself at M = 1): 2^-23 relative on running_var,
             2^-23 (|(1 - m) r| + |m mu|) on running_mean.
  bn_act     v = (z - mean) invstd gamma + beta: four roundings (a contracted multiply-add counted as one): 2^-21 (|zh gamma| + |beta|), zh in
             float64; ReLU and tanh are 1-Lipschitz; tanh adds FLOOR = 1e-6, the project's floor of one gate-function evaluation
             (tests/lstm_step_ref.py).  y_drop: 0 where keep == 0, keep_scale times the bound elsewhere.
  bn_bwd     dz = gamma invstd (dy - dbeta / M - zh dgamma / M) with dbeta, dgamma the float32 INPUTS: 2^-21 |gamma invstd| (|dy| + |dbeta| / M +
             |zh dgamma| / M).  acc += d*: the float32 sum, bit for bit.
  act        forward 2^-22 |ref| (+ FLOOR keep_scale for tanh / sigmoid); backward from the saved activation 2^-22 |ref|: two roundings for the
             identity, ReLU and tanh (1 - y y contracted, then the product); the sigmoid's y (1 - y) has 1 - y (half an ulp at most: exact for
             y >= 1/2, a result in [1/2, 1] otherwise) and two products, 2.5 u of the bound's 4 u (ACT_BWD_SIGMOID_SHARE).
  colsum     terms in float32, float64 within a block of rows_per_block(M) rows, one float32 atomic per block:
             (ceil(M / rpb) + 6) u (|out_before| + sum_m |t_m|) per column.
  conv1d_in1_dw  float32 accumulation, <= 16 rows per thread + 3 partial adds, one atomic per 64-row block: (19 + ceil(M / 64)) u (|before| + sum |term|).
  unpack     2^-23 (|dw_before| + |dwp scale|).
  concat_spk columns [0, C) a copy; the rest (ceil(S / 64) + 12) u |ref| (an all-zero vector: exact zeros).
  layernorm  the project's own tolerances for these input distributions (tests/test_gpu_parity.py, tests/test_gpu_backward.py): y 2e-5 keep_scale,
             scalar head 5e-5 keep_scale, dx 2e-4; parameter gradients (float32 sums over a wave's rows, one atomic per wave):
             (R + W + 8) u (|before| + sum_rows |term|), W = min(M, 4 min(ceil(M / 4), 256)) waves, R = ceil(M / W) rows per wave.
The f32_* functions evaluate the same expressions in float32 numpy in the kernels' order of operations (a contracted multiply-add where the
expression is 1 - v v or an accumulation a + b c: one rounding, modelled through float64): the arithmetic-precision model of the bounds
(test_train_pointwise_ref_cpu.py: at most half of every bound)."""
import zlib

import numpy as np

U = 2.0 ** -24
FLOOR = 1e-6
ACT_NONE, ACT_RELU, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3
BN_EPS, LN_EPS, KEEP_SCALE, MOMENTUM = 1e-5, 1e-12, 2.0, 0.1
ACT_BWD_SIGMOID_SHARE = 0.625  # the worst case of the float32 sigmoid backward as a share of its 2^-22 bound (see above): not within one half
TWIN_OFFSET = 1  # floats: operand views this far into a 16-byte aligned buffer are 4-byte but not 16-byte aligned (the scalar twin of a four-wide kernel)
f32 = np.float32


def f64(x):
    return None if x is None else np.asarray(x, dtype=np.float64)


def wide(v):
    """a `float` argument as the kernel sees it"""
    return float(np.float32(v))


def rng_of(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def rows_per_block(m):
    """rows of one block of the column reductions (colsum, bn_stats)"""
    return 128 if m >= 8192 else 64


def act_f64(v, act):
    if act == ACT_RELU:
        return np.maximum(v, 0.0)
    if act == ACT_TANH:
        return np.tanh(v)
    if act == ACT_SIGMOID:
        return 1.0 / (1.0 + np.exp(-v))
    return v


def act_f32(v, act):
    assert v.dtype == f32
    if act == ACT_RELU:
        return np.maximum(v, f32(0))
    if act == ACT_TANH:
        return np.tanh(v)
    if act == ACT_SIGMOID:
        return f32(1) / (f32(1) + np.exp(-v))
    return v


def fma32(a, b, c):
    """a * b + c rounded once (float32 operands: the product is exact in float64)"""
    return (f64(a) * f64(b) + f64(c)).astype(f32)


def keep_factor(keep, keep_scale, shape):
    return np.ones(shape) if keep is None else np.where(np.asarray(keep) != 0, wide(keep_scale), 0.0)


# ---- train-mode BatchNorm --------------------------------------------------------------------------------------------------------------------
def ref_bn_stats(z, eps=BN_EPS, momentum=MOMENTUM, running_mean=None, running_var=None):
    z = f64(z)
    m = z.shape[0]
    mu = z.sum(0) / m
    var = ((z - mu) ** 2).sum(0) / m
    out = dict(mean=mu, var=var, invstd=1.0 / np.sqrt(var + wide(eps)))
    if running_mean is not None:
        mom = wide(momentum)
        unbiased = var * m / (m - 1) if m > 1 else var
        out.update(running_mean=(1.0 - mom) * f64(running_mean) + mom * mu, running_var=(1.0 - mom) * f64(running_var) + mom * unbiased)
    return out


def bound_bn_stats(z, ref, momentum=MOMENTUM, running_mean=None):
    b = dict(mean=2.0 ** -23 * np.abs(ref["mean"]) + 1e-12 * np.abs(f64(z)).mean(0), invstd=2.0 ** -23 * ref["invstd"])
    if running_mean is not None:
        mom = wide(momentum)
        b.update(running_mean=2.0 ** -23 * (np.abs((1.0 - mom) * f64(running_mean)) + np.abs(mom * ref["mean"])), running_var=2.0 ** -23 * np.abs(ref["running_var"]))
    return b


def f32_bn_stats(z, eps=BN_EPS, momentum=MOMENTUM, running_mean=None, running_var=None):
    """float64 sums and sums of squares, var = Q / M - mu^2 clamped at 0, every output rounded once"""
    z = f64(z)
    m = z.shape[0]
    mu = z.sum(0) / m
    var = np.maximum((z * z).sum(0) / m - mu * mu, 0.0)
    out = dict(mean=mu.astype(f32), invstd=(1.0 / np.sqrt(var + wide(eps))).astype(f32))
    if running_mean is not None:
        mom = wide(momentum)
        unbiased = var * m / (m - 1) if m > 1 else var
        out.update(running_mean=((1.0 - mom) * f64(running_mean) + mom * mu).astype(f32), running_var=((1.0 - mom) * f64(running_var) + mom * unbiased).astype(f32))
    return out


def ref_bn_act(z, mean, invstd, gamma, beta, act, keep=None, keep_scale=1.0):
    zh = (f64(z) - f64(mean)) * f64(invstd)
    v = act_f64(zh * f64(gamma) + f64(beta), act)
    return dict(zh=zh, y_act=v, y_drop=v * keep_factor(keep, keep_scale, v.shape))


def bound_bn_act(ref, gamma, beta, act, keep=None, keep_scale=1.0):
    b = 2.0 ** -21 * (np.abs(ref["zh"] * f64(gamma)) + np.abs(f64(beta))) + (FLOOR if act == ACT_TANH else 0.0)
    return dict(y_act=b, y_drop=b * keep_factor(keep, keep_scale, b.shape))


def f32_bn_act(z, mean, invstd, gamma, beta, act, keep=None, keep_scale=1.0):
    v = act_f32(((z - mean) * invstd) * gamma + beta, act)
    assert v.dtype == f32
    vd = v if keep is None else np.where(np.asarray(keep) != 0, v * f32(keep_scale), f32(0))
    return dict(y_act=v, y_drop=vd)


def bn_param_grads(dy, z, mean, invstd):
    """(dbeta, dgamma) of this batch in float64, rounded to the float32 the backward kernel receives"""
    zh = (f64(z) - f64(mean)) * f64(invstd)
    return f64(dy).sum(0).astype(f32), (f64(dy) * zh).sum(0).astype(f32)


def ref_bn_bwd(dy, z, mean, invstd, gamma, dbeta, dgamma, acc=None):
    m = z.shape[0]
    zh = (f64(z) - f64(mean)) * f64(invstd)
    out = dict(zh=zh, dz=f64(gamma) * f64(invstd) * (f64(dy) - f64(dbeta) / m - zh * f64(dgamma) / m))
    if acc is not None:  # the float32 sum, bit for bit
        out.update(acc_dbeta=np.asarray(acc[0], f32) + np.asarray(dbeta, f32), acc_dgamma=np.asarray(acc[1], f32) + np.asarray(dgamma, f32))
    return out


def bound_bn_bwd(ref, dy, invstd, gamma, dbeta, dgamma):
    m = dy.shape[0]
    return 2.0 ** -21 * np.abs(f64(gamma) * f64(invstd)) * (np.abs(f64(dy)) + np.abs(f64(dbeta)) / m + np.abs(ref["zh"] * f64(dgamma)) / m)


def f32_bn_bwd(dy, z, mean, invstd, gamma, dbeta, dgamma):
    inv_m = f32(1) / f32(z.shape[0])
    zh = (z - mean) * invstd
    g = (gamma * invstd) * ((dy - dbeta * inv_m) - (zh * dgamma) * inv_m)
    assert g.dtype == f32
    return g


# ---- activation maps -------------------------------------------------------------------------------------------------------------------------
def ref_act_fwd(x, act, keep=None, keep_scale=1.0):
    return act_f64(f64(x), act) * keep_factor(keep, keep_scale, np.shape(x))


def bound_act_fwd(ref, act, keep=None, keep_scale=1.0):
    floor = FLOOR if act in (ACT_TANH, ACT_SIGMOID) else 0.0
    return 2.0 ** -22 * np.abs(ref) + floor * keep_factor(keep, keep_scale, ref.shape)


def f32_act_fwd(x, act, keep=None, keep_scale=1.0):
    v = act_f32(x, act)
    return v if keep is None else np.where(np.asarray(keep) != 0, v * f32(keep_scale), f32(0))


def ref_act_bwd(dy, y, act, keep=None, keep_scale=1.0):
    g, y = f64(dy) * keep_factor(keep, keep_scale, np.shape(dy)), f64(y)
    if act == ACT_RELU:
        return np.where(y > 0, g, 0.0)
    if act == ACT_TANH:
        return g * (1.0 - y * y)
    if act == ACT_SIGMOID:
        return g * y * (1.0 - y)
    return g


def bound_act_bwd(ref):
    return 2.0 ** -22 * np.abs(ref)


def f32_act_bwd(dy, y, act, keep=None, keep_scale=1.0):
    g = dy if keep is None else np.where(np.asarray(keep) != 0, dy * f32(keep_scale), f32(0))
    if act == ACT_RELU:
        g = np.where(y > 0, g, f32(0))
    elif act == ACT_TANH:
        g = g * fma32(-y, y, f32(1))
    elif act == ACT_SIGMOID:
        g = g * (y * (f32(1) - y))
    assert g.dtype == f32
    return g


# ---- column sums -----------------------------------------------------------------------------------------------------------------------------
def colsum_terms(x, y=None, g=None, b=None, mode=0):
    """mode 0: x; 1: x y; 2: x (y - b) / g; 3: x (y - b) g   (g, b per column)"""
    x = f64(x)
    if mode == 0:
        return x
    if mode == 1:
        return x * f64(y)
    d = f64(y) - f64(b)[None, :]
    return x * d / f64(g)[None, :] if mode == 2 else x * d * f64(g)[None, :]


def ref_colsum(terms, before):
    return f64(before) + terms.sum(0)


def bound_colsum(terms, before):
    m = terms.shape[0]
    return (-(-m // rows_per_block(m)) + 6) * U * (np.abs(f64(before)) + np.abs(terms).sum(0))


def f32_colsum(x, y, g, b, mode, before):
    if mode == 0:
        t = x
    elif mode == 1:
        t = x * y
    else:
        t = x * ((y - b[None, :]) * ((f32(1) / g) if mode == 2 else g)[None, :])
    assert t.dtype == f32
    out, rpb = np.array(before, f32), rows_per_block(x.shape[0])
    for lo in range(0, x.shape[0], rpb):
        out = out + f64(t[lo: lo + rpb]).sum(0).astype(f32)
    assert out.dtype == f32
    return out


# ---- Conv1d(1 -> C, k) weight / bias gradient ---------------------------------------------------------------------------------------------------
def conv_in1_taps(x, k, seg_lo=None, seg_hi=None):
    """XS [M, k]: XS[m, j] = x[m + j - pad] where that row lies inside [seg_lo[m], seg_hi[m]) (the whole range without bounds), else 0"""
    m = len(x)
    lo = np.zeros(m, np.int64) if seg_lo is None else np.asarray(seg_lo, np.int64)
    hi = np.full(m, m, np.int64) if seg_hi is None else np.asarray(seg_hi, np.int64)
    src = np.arange(m)[:, None] + np.arange(k)[None, :] - (k - 1) // 2
    ok = (src >= lo[:, None]) & (src < hi[:, None])
    return np.where(ok, np.asarray(x)[np.clip(src, 0, m - 1)], 0).astype(np.asarray(x).dtype)


def ref_conv1d_in1_dw(dy, x, k, dw_before, db_before=None, seg_lo=None, seg_hi=None):
    """dy [M, C] (the columns the kernel owns), x [M]; returns dict(dw [C, k], db [C], and the bounds)"""
    dy, xs = f64(dy), f64(conv_in1_taps(x, k, seg_lo, seg_hi))
    m = dy.shape[0]
    fac = (19 + -(-m // 64)) * U
    out = dict(dw=f64(dw_before) + dy.T @ xs, bound_dw=fac * (np.abs(f64(dw_before)) + np.abs(dy).T @ np.abs(xs)))
    if db_before is not None:
        out.update(db=f64(db_before) + dy.sum(0), bound_db=fac * (np.abs(f64(db_before)) + np.abs(dy).sum(0)))
    return out


def f32_conv1d_in1_dw(dy, x, k, dw_before, db_before, seg_lo=None, seg_hi=None):
    """float32 multiply-adds over the rows m_lo + ty, + 4, ... of a 64-row block (ty = 0..3), (p0 + p1) + (p2 + p3), one float32 add per block"""
    xs = conv_in1_taps(x, k, seg_lo, seg_hi)
    m, c = dy.shape
    dw, db = np.array(dw_before, f32), np.array(db_before, f32)
    for m_lo in range(0, m, 64):
        pw, pb = np.zeros((4, c, k), f32), np.zeros((4, c), f32)
        for r in range(m_lo, min(m, m_lo + 64)):
            ty = (r - m_lo) % 4
            pw[ty] = fma32(dy[r][:, None], xs[r][None, :], pw[ty])
            pb[ty] = pb[ty] + dy[r]
        dw = dw + ((pw[0] + pw[1]) + (pw[2] + pw[3]))
        db = db + ((pb[0] + pb[1]) + (pb[2] + pb[3]))
    assert dw.dtype == f32 and db.dtype == f32
    return dw, db


# ---- tap-major gradient unpack -----------------------------------------------------------------------------------------------------------------
def ref_unpack(dwp, dw_before, scale=None):
    """dw[co, ci, j] += dwp[j, co, ci] * scale[co]; returns (dw, bound)"""
    t = np.transpose(f64(dwp), (1, 2, 0)) * (1.0 if scale is None else f64(scale)[:, None, None])
    return f64(dw_before) + t, 2.0 ** -23 * (np.abs(f64(dw_before)) + np.abs(t))


def f32_unpack(dwp, dw_before, scale=None):
    """dw + dwp * scale as one contracted multiply-add"""
    return fma32(np.transpose(dwp, (1, 2, 0)), f32(1) if scale is None else scale[:, None, None], dw_before)


# ---- speaker concat --------------------------------------------------------------------------------------------------------------------------
def ref_concat_spk(hs, spk, t):
    """hs [M, C] (any row stride), spk [B, S]: cat[hs, spk[row // t] / max(||spk[row // t]||_2, 1e-12)]; returns (out [M, C + S], bound)"""
    hs, spk = f64(hs), f64(spk)
    m, c = hs.shape
    s = spk.shape[1]
    unit = spk / np.maximum(np.sqrt((spk * spk).sum(1, keepdims=True)), 1e-12)
    out = np.concatenate([hs, unit[np.arange(m) // t]], axis=1)
    bound = np.zeros_like(out)
    bound[:, c:] = (-(-s // 64) + 12) * U * np.abs(out[:, c:])
    return out, bound


def wave_sum32(v):
    """the xor-butterfly sum over the 64 lanes of a wave, float32: v [R, 64] -> [R]"""
    assert v.dtype == f32 and v.shape[1] == 64
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ o]
    return v[:, 0]


def lanes_of(a, per=None):
    """[R, C] -> [R, per, 64] zero padded: element (i, lane) = column lane + 64 i"""
    r, c = a.shape
    per = -(-c // 64) if per is None else per
    out = np.zeros((r, per * 64), a.dtype)
    out[:, :c] = a
    return out.reshape(r, per, 64)


def f32_concat_spk(hs, spk, t):
    m = hs.shape[0]
    sl = lanes_of(spk)
    q = np.zeros((spk.shape[0], 64), f32)
    for i in range(sl.shape[1]):
        q = fma32(sl[:, i], sl[:, i], q)
    inv = f32(1) / np.maximum(np.sqrt(wave_sum32(q)), f32(1e-12))
    return np.concatenate([hs, (spk * inv[:, None])[np.arange(m) // t]], axis=1).astype(f32)


# ---- channel LayerNorm (+ dropout, Linear(C -> 1) head, pad mask) ---------------------------------------------------------------------------------
LN_TOL_Y, LN_TOL_S, LN_TOL_DX = 2e-5, 5e-5, 2e-4


def ln_waves(m):
    """(W waves, R rows per wave at most) of the backward launch: 4 waves per block, at most 256 blocks"""
    w = min(m, 4 * min(-(-m // 4), 256))
    return w, -(-m // w)


def ln_maxper(c):
    """columns per lane of the kernel arm that takes C"""
    return 1 if c <= 64 else 4 if c <= 256 else 8 if c <= 512 else 16


def ref_layernorm(x, gamma, beta, eps=LN_EPS, keep=None, keep_scale=1.0, lin_w=None, lin_b=None, pad=None):
    x = f64(x)
    mu = x.mean(1, keepdims=True)
    rstd = 1.0 / np.sqrt(((x - mu) ** 2).mean(1, keepdims=True) + wide(eps))
    xh = (x - mu) * rstd
    ks = keep_factor(keep, keep_scale, x.shape)
    y = (xh * f64(gamma) + f64(beta)) * ks
    out = dict(xh=xh, rstd=rstd, ks=ks, y=y, tol_y=LN_TOL_Y * wide(keep_scale) * (ks != 0))
    if lin_w is not None:
        live = np.ones(x.shape[0], bool) if pad is None else np.asarray(pad) == 0
        out.update(scalar=np.where(live, y @ f64(lin_w) + float(f64(lin_b).reshape(-1)[0]), 0.0), tol_s=LN_TOL_S * wide(keep_scale) * live)
    return out


def _ln_rows32(x, per):
    """(mean, rstd-less centred values) as the kernels form them: lane-strided float32 sums + butterfly"""
    c = x.shape[1]
    xl = lanes_of(x, per)
    s = np.zeros((x.shape[0], 64), f32)
    for i in range(per):
        s = s + xl[:, i]
    mean = wave_sum32(s) / f32(c)
    d = np.where(lanes_of(np.ones_like(x), per) != 0, xl - mean[:, None, None], f32(0))
    q = np.zeros((x.shape[0], 64), f32)
    for i in range(per):
        q = q + d[:, i] * d[:, i]
    return mean, wave_sum32(q) / f32(c)


def f32_layernorm(x, gamma, beta, eps=LN_EPS, keep=None, keep_scale=1.0, lin_w=None, lin_b=None, pad=None):
    per = ln_maxper(x.shape[1])
    mean, var = _ln_rows32(x, per)
    rstd = f32(1) / np.sqrt(var + f32(eps))
    o = ((x - mean[:, None]) * rstd[:, None]) * gamma + beta
    if keep is not None:
        o = np.where(np.asarray(keep) != 0, o * f32(keep_scale), f32(0))
    assert o.dtype == f32
    out = dict(y=o)
    if lin_w is not None:
        pl = lanes_of(o * lin_w, per)
        dot = np.zeros((x.shape[0], 64), f32)
        for i in range(per):
            dot = dot + pl[:, i]
        sc = wave_sum32(dot) + np.asarray(lin_b, f32).reshape(-1)[0]
        out["scalar"] = sc if pad is None else np.where(np.asarray(pad) != 0, f32(0), sc)
    return out


def ref_layernorm_bwd(x, gamma, beta, eps=LN_EPS, dy=None, lin_w=None, ds=None, pad=None, keep=None, keep_scale=1.0, before=None):
    """Gradients of L = sum(y_drop * dy) + sum(s * ds), s the masked head of ref_layernorm.  before: dict of the accumulators' contents
    (dgamma, dbeta, dlin_w, dlin_b).  Returns dx, the four accumulators after the call, and bound_* for each."""
    fw = ref_layernorm(x, gamma, beta, eps, keep, keep_scale)
    xh, rstd, ks = fw["xh"], fw["rstd"], fw["ks"]
    m = xh.shape[0]
    dsr = np.zeros(m) if ds is None else f64(ds) * (1.0 if pad is None else (np.asarray(pad) == 0))
    gy = (np.zeros_like(xh) if dy is None else f64(dy)) * ks
    if ds is not None:
        gy = gy + dsr[:, None] * f64(lin_w)[None, :] * ks
    dxh = gy * f64(gamma)
    dx = rstd * (dxh - dxh.mean(1, keepdims=True) - xh * (dxh * xh).mean(1, keepdims=True))
    terms = dict(dgamma=gy * xh, dbeta=gy)
    if ds is not None:
        terms.update(dlin_w=dsr[:, None] * fw["y"], dlin_b=dsr[:, None])
    w, r = ln_waves(m)
    out = dict(dx=dx, bound_dx=LN_TOL_DX * np.any(gy != 0, axis=1, keepdims=True) * np.ones_like(dx))
    for k, t in terms.items():
        out[k] = f64(before[k]) + t.sum(0)
        out["bound_" + k] = (r + w + 8) * U * (np.abs(f64(before[k])) + np.abs(t).sum(0))
    return out


def f32_layernorm_bwd(x, gamma, beta, eps=LN_EPS, dy=None, lin_w=None, ds=None, pad=None, keep=None, keep_scale=1.0, before=None):
    m, c = x.shape
    per = ln_maxper(c)
    mean, var = _ln_rows32(x, per)
    rstd = (f32(1) / np.sqrt(var + f32(eps)))[:, None]
    xh = (x - mean[:, None]) * rstd
    ks = np.ones((m, c), f32) if keep is None else np.where(np.asarray(keep) != 0, f32(keep_scale), f32(0))
    dsr = np.zeros(m, f32) if ds is None else (ds if pad is None else np.where(np.asarray(pad) != 0, f32(0), ds))
    g = np.zeros((m, c), f32) if dy is None else dy
    terms = {}
    if ds is not None:
        g = g + dsr[:, None] * lin_w[None, :]
        terms["dlin_w"] = (dsr[:, None] * (xh * gamma + beta)) * ks
        terms["dlin_b"] = dsr[:, None]
    g = g * ks
    terms.update(dgamma=g * xh, dbeta=g)

    def rowsum(v):
        vl = lanes_of(v, per)
        s = np.zeros((m, 64), f32)
        for i in range(per):
            s = s + vl[:, i]
        return (wave_sum32(s) / f32(c))[:, None]

    a1, a2 = rowsum(g * gamma), rowsum((g * gamma) * xh)
    out = dict(dx=rstd * ((g * gamma - a1) - xh * a2))
    w, _ = ln_waves(m)
    for k, t in terms.items():
        acc = np.array(before[k], f32)
        for w0 in range(w):  # one wave: its rows in order into a register, then one atomic
            part = np.zeros(t.shape[1], f32)
            for row in range(w0, m, w):
                part = part + t[row]
            acc = acc + part
        out[k] = acc
    assert all(v.dtype == f32 for v in out.values())
    return out


# ---- seeded inputs and the case tables ---------------------------------------------------------------------------------------------------------------
def rnd(rng, *shape):
    return rng.standard_normal(shape).astype(f32)


def offset_data(rng, m, c):
    """0.7 N(0,1) around per-column offsets drawn from {0, 3, 100}"""
    off = rng.choice(np.array([0.0, 3.0, 100.0]), size=c)
    return (0.7 * rng.standard_normal((m, c)) + off[None, :]).astype(f32), off


# id: (M, C, momentum, running buffers given)
BN_STATS_CASES = {"m1_c1": (1, 1, 0.1, True), "m2_c65": (2, 65, 0.1, True), "m63_c64": (63, 64, 1.0, True), "m65_c130": (65, 130, 0.1, True),
                  "m257_c7": (257, 7, 0.1, False), "m8193_c65": (8193, 65, 0.1, True)}
BN_CONST = 3.25  # the value of the constant column (C // 2): var = 0, invstd = 1 / sqrt(eps)


def bn_stats_inputs(cid):
    m, c, mom, run = BN_STATS_CASES[cid]
    rng = rng_of("bn_stats", cid)
    z, off = offset_data(rng, m, c)
    z[:, c // 2] = f32(BN_CONST)
    return dict(m=m, c=c, momentum=mom, z=z, off=off, const_col=c // 2, running_mean=rnd(rng, c) if run else None,
                running_var=(0.5 + rng.random_sample(c)).astype(f32) if run else None)


BN_SHAPES = ((3, 5), (67, 70), (67, 132), (33, 96))  # bn_act and bn_bwd: two scalar (C % 4 != 0), two four-wide; planes at C = 96
BN_ACTS = (ACT_NONE, ACT_RELU, ACT_TANH)


def bn_inputs(m, c):
    """z around offsets with its own float64 statistics rounded to float32, affine parameters, the incoming gradient and its float32 parameter
    gradients, a keep mask, the accumulators' contents"""
    rng = rng_of("bn", m, c)
    z, _ = offset_data(rng, m, c)
    st = ref_bn_stats(z)
    mean, invstd = st["mean"].astype(f32), st["invstd"].astype(f32)
    dy = rnd(rng, m, c)
    dbeta, dgamma = bn_param_grads(dy, z, mean, invstd)
    return dict(m=m, c=c, z=z, mean=mean, invstd=invstd, gamma=(1 + 0.1 * rnd(rng, c)).astype(f32), beta=rnd(rng, c), dy=dy, dbeta=dbeta, dgamma=dgamma,
                keep=(rng.random_sample((m, c)) < 0.5).astype(np.uint8), acc_dbeta=rnd(rng, c), acc_dgamma=rnd(rng, c))


ACT_SHAPES = ((7, 5), (33, 96))  # n = 35: the scalar forward kernel; 33 x 96: four-wide, with planes
ACTS = (ACT_NONE, ACT_RELU, ACT_TANH, ACT_SIGMOID)


def act_inputs(r, c):
    rng = rng_of("act", r, c)
    x = (1.5 * rnd(rng, r, c)).astype(f32)
    return dict(x=x, dy=rnd(rng, r, c), keep=(rng.random_sample((r, c)) < 0.5).astype(np.uint8), y={a: act_f64(f64(x), a).astype(f32) for a in ACTS})


COLSUM_SHAPES = ((1, 1), (67, 65), (300, 130), (8193, 70))


def colsum_inputs(m, c):
    rng = rng_of("colsum", m, c)
    return dict(x=rnd(rng, m, c), y=(rnd(rng, m, c) + f32(0.5)).astype(f32), g=(1 + 0.1 * rnd(rng, c)).astype(f32), b=rnd(rng, c), out=rnd(rng, c), out_x=rnd(rng, c))


# (M, C, k, ldy, segment bounds and db given)
CONV_DW_CASES = ((1, 1, 1, 1, True), (70, 65, 9, 72, True), (333, 130, 15, 130, True), (200, 64, 9, 64, False))
SEG_PATTERN = (3, 1, 50, 16)


def seg_lens(m):
    """SEG_PATTERN tiled to m rows (the last segment cut short)"""
    lens = []
    while sum(lens) < m:
        lens.append(min(SEG_PATTERN[len(lens) % len(SEG_PATTERN)], m - sum(lens)))
    return lens


def seg_bounds(lens):
    off = np.concatenate([[0], np.cumsum(lens)])
    return np.repeat(off[:-1], lens).astype(np.int32), np.repeat(off[1:], lens).astype(np.int32)


def conv_dw_inputs(m, c, k, ldy, full):
    """dy_buf [M, ldy]: the gradient in columns [0, C), NaN in the padding columns (never read)"""
    rng = rng_of("conv_dw", m, c, k)
    dy_buf = np.full((m, ldy), np.nan, f32)
    dy_buf[:, :c] = rnd(rng, m, c)
    lo, hi = seg_bounds(seg_lens(m)) if full else (None, None)
    return dict(dy_buf=dy_buf, x=rnd(rng, m), seg_lo=lo, seg_hi=hi, dw=rnd(rng, c, 1, k), db=rnd(rng, c) if full else None)


UNPACK_SHAPES = ((5, 3, 3), (70, 33, 5))  # (cout, cin, k)


def unpack_inputs(cout, cin, k):
    rng = rng_of("unpack", cout, cin, k)
    return dict(dwp=rnd(rng, k, cout, cin), dw=rnd(rng, cout, cin, k), scale=(1 + 0.5 * rnd(rng, cout)).astype(f32))


# (B, T, C, S, M, ldh, planes, kinds of the speaker rows)
CONCAT_CASES = ((3, 7, 20, 12, 21, 20, False, ("unit", "large", "tiny")), (2, 5, 48, 16, 8, 56, True, ("zero", "unit")))
SPK_SCALE = dict(unit=1.0, large=1e3, tiny=1e-13, zero=0.0)  # tiny: a norm below the 1e-12 clamp


def concat_inputs(b, t, c, s, m, ldh, planes, kinds):
    """hs_buf [M, ldh]: hs in columns [0, C), NaN beyond"""
    rng = rng_of("concat", b, t, c, s)
    hs_buf = np.full((m, ldh), np.nan, f32)
    hs_buf[:, :c] = rnd(rng, m, c)
    spk = np.stack([(SPK_SCALE[kd] * rng.standard_normal(s)).astype(f32) for kd in kinds])
    return dict(hs_buf=hs_buf, spk=spk)


LN_FWD_CASES = ((9, 20), (9, 64), (9, 65), (9, 257), (9, 520))
# (M, C, dy given, ds given)
LN_BWD_CASES = ((9, 65, True, True), (9, 257, False, True), (9, 513, True, False), (1029, 20, True, True))


def ln_inputs(m, c):
    """the distributions of tests/test_gpu_backward.py::test_layernorm_bwd_with_scalar_head; row 1 is dropped whole, row 0 is live, the last row padding"""
    rng = rng_of("ln", m, c)
    d = dict(x=(2 * rnd(rng, m, c) + f32(0.5)).astype(f32), gamma=(1 + 0.1 * rnd(rng, c)).astype(f32), beta=rnd(rng, c),
             lin_w=(rnd(rng, c) / np.sqrt(c)).astype(f32), lin_b=rnd(rng, 1), dy=rnd(rng, m, c), ds=rnd(rng, m),
             pad=(rng.random_sample(m) < 0.2).astype(np.uint8), keep=(rng.random_sample((m, c)) < 0.5).astype(np.uint8),
             before=dict(dgamma=rnd(rng, c), dbeta=rnd(rng, c), dlin_w=rnd(rng, c), dlin_b=rnd(rng, 1)))
    d["pad"][0], d["pad"][-1] = 0, 1
    d["keep"][1] = 0
    return d
