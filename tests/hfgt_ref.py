"""Float64 numpy statement of the HiFi-GAN generator's training launches -- the convolution, the transposed convolution, a residual unit, a stage and
input_conv + the stages -- forward and backward on packed rows, with derived worst-case bounds (the contract of include/fcl_hip.h
"HiFi-GAN generator, training form").  Arrays are packed [rows, C] with the utterance lengths `lens` (rows of the array's own rate); weights are in
torch's orientation: Conv1d (cout, cin, k), ConvTranspose1d (cin, cout, 2 s).

Bounds, u = 2^-24.  A contraction of K products evaluated in float32 in any order is within (K + c) u sum |w| |x| of its exact value, c counting the
roundings around it (the LeakyReLU product on load, the bias, the residual); an input error e propagates as |w| e, through LeakyReLU unchanged (it is
1-Lipschitz).  A sum over n rows: (n + 2) u sum |.| |.|.  No transcendental function runs on the device, so no measured constant appears.  Every function
takes the input errors (None: exact inputs) -- with None it gives the first term, the bound of one launch on given inputs.

The mask m(v) = 1 where v > 0, else the slope, jumps at 0.  A cell whose float64 pre-activation is no larger than its own bound may take either value on
the device: there the product m * S is uncertain by its whole jump (1 - slope) (|S| + e_S), which is added to that cell's bound and so enters every sum
taken from it.  `unsure` counts such cells; the tests assert that they are at most MASK_CAP of an array."""
import math

import numpy as np

import hifigan_ref as H

U = 2.0 ** -24
MASK_CAP = 0.01
LENS = (1, 5, 130, 1100, 77)  # pwgt_ref.LENS: an utterance shorter than the 25-row halo, edges inside a 128-row tile, one across a 1 024-row chunk
SLOPE = float(np.float32(0.1))  # the slope the device multiplies by
CONV_CELLS = [(k, d, c) for k in (3, 7, 11) for d in (1, 5) for c in (32, 64, 128, 256)]
UNIT_CELLS = [(3, 1, 32), (11, 5, 32), (7, 3, 64)]
TCONV_CELLS = list(zip(H.TCONV_SCALES, H.TCONV_CIN, H.TCONV_LENS))
# the stage and whole-module cases: hifigan_ref.SMALL with two blocks of two units.  The running bound grows with every matrix's absolute row sums
# (0.8 gain sqrt(K) per convolution at random_state_dict's N(0, gain^2 / fan_in)): at a quarter of its gain the last stage's bound is above the array's
# peak and 94 % of the mask cells are unsure, at 1 / 8 2.5 % are, at 1 / 16 the mel gradient's bound is still above its peak; at 1 / 32 every bound is
# below its array's peak and 0.04 % of the cells of the worst array are unsure
SMALL = dict(H.SMALL, resblock_kernel_sizes=(3, 7), resblock_dilations=((1, 3), (1, 5)))
GAIN = 1.0 / 32
MUTANTS = ("taps_not_reversed", "mask_dropped", "mask_slope_zero", "no_residual_in_dx", "no_seed_scale", "conv2_dilated", "phase_off_by_one",
           "tconv_across_edge", "missing_bias_gradient")


def shift(a, lens, sh, across=False):
    """rows t -> a[t + sh], zero where t + sh leaves row t's utterance (across: the batch is treated as one utterance -- a mutant)"""
    out = np.zeros_like(a)
    off = 0
    for n in ([len(a)] if across else lens):
        if abs(sh) < n:
            if sh >= 0:
                out[off : off + n - sh] = a[off + sh : off + n]
            else:
                out[off - sh : off + n] = a[off : off + n + sh]
        off += n
    return out


def a64(v):
    return np.abs(np.asarray(v, dtype=np.float64))


def _z(e, like):
    return np.zeros(np.shape(like)) if e is None else e


def lrelu(v, slope):
    return np.where(v > 0, v, v * v.dtype.type(slope))


def mask(v, slope, mutant=None):
    if mutant == "mask_dropped":
        return np.ones_like(v)
    return np.where(v > 0, v.dtype.type(1.0), v.dtype.type(0.0 if mutant == "mask_slope_zero" else slope))


def conv_fwd(x, w, b, dil, lens, slope=SLOPE, act=True, res=None, ex=None, eres=None, dt=np.float64):
    """y = b + sum_j op(x)[t + (j - h) dil] W_j^T (+ res), op = LeakyReLU when act -> (y, e_y)"""
    f = lambda v: np.asarray(v, dtype=dt)
    k, cin = w.shape[2], w.shape[1]
    a = lrelu(f(x), slope) if act else f(x)
    y, ay, ein = np.tile(f(b), (len(x), 1)), np.tile(a64(b), (len(x), 1)), np.zeros((len(x), w.shape[0]))
    for j in range(k):
        sh, Wj = (j - (k - 1) // 2) * dil, w[:, :, j].T
        y = y + shift(a, lens, sh) @ f(Wj)
        ay += shift(a64(a), lens, sh) @ a64(Wj)
        if ex is not None:
            ein += shift(ex, lens, sh) @ a64(Wj)
    if res is not None:
        y = y + f(res)
        ay, ein = ay + a64(res), ein + _z(eres, res)
    return y, (k * cin + 3) * U * ay + ein


def masked(S, aS, eS, pre, slope, carry=None, epre=None, ecarry=None, mutant=None, dt=np.float64):
    """m(pre) * S + carry -> (value, bound, share of the cells whose mask is unsure)"""
    f = lambda v: np.asarray(v, dtype=dt)
    if pre is None:
        v, e, unsure = S, eS.copy(), 0.0
    else:
        v = mask(f(pre), slope, mutant) * S
        e = eS + U * a64(v)
        cells = a64(pre) <= _z(epre, pre) if epre is not None else np.zeros(np.shape(pre), bool)
        e = e + cells * (1.0 - slope) * (a64(S) + eS)
        unsure = float(cells.mean())
    if carry is not None and mutant != "no_residual_in_dx":
        v = v + f(carry)
        e = e + _z(ecarry, carry) + U * a64(v)
    return v, e, unsure


def conv_dx(g, w, dil, lens, slope=SLOPE, pre=None, carry=None, eg=None, epre=None, ecarry=None, mutant=None, dt=np.float64):
    """dx = m(pre) * sum_j g[t - (j - h) dil] W_j + carry; g [rows, cout], w (cout, cin, k) -> (dx [rows, cin], e_dx, unsure)"""
    f = lambda v: np.asarray(v, dtype=dt)
    k, cout = w.shape[2], w.shape[0]
    S, aS, eS = np.zeros((len(g), w.shape[1]), dt), np.zeros((len(g), w.shape[1])), np.zeros((len(g), w.shape[1]))
    for j in range(k):
        sh, Wj = (j - (k - 1) // 2) * dil, w[:, :, j]
        S = S + shift(f(g), lens, sh if mutant == "taps_not_reversed" else -sh) @ f(Wj)
        aS += shift(a64(g), lens, -sh) @ a64(Wj)
        if eg is not None:
            eS += shift(eg, lens, -sh) @ a64(Wj)
    eS = (k * cout + 1) * U * aS + eS
    return masked(S, aS, eS, pre, slope, carry, epre, ecarry, mutant, dt)


def conv_dw(x, g, k, dil, lens, slope=SLOPE, act=True, ex=None, eg=None, mutant=None, dt=np.float64):
    """dW[:, :, j] = sum_t g[t]^T op(x)[t + (j - h) dil], db = sum_t g[t] -> (dW (cout, cin, k), db, e_dW, e_db)"""
    f = lambda v: np.asarray(v, dtype=dt)
    n, cin, cout = len(x), x.shape[1], g.shape[1]
    a = lrelu(f(x), slope) if act else f(x)
    ea, eg_ = _z(ex, x), _z(eg, g)
    dW, eW = np.zeros((cout, cin, k), dt), np.zeros((cout, cin, k))
    for j in range(k):
        sh = (j - (k - 1) // 2) * dil
        a_s, aa, ee = shift(a, lens, sh), shift(a64(a), lens, sh), shift(ea, lens, sh)
        dW[:, :, j] = f(g).T @ a_s
        eW[:, :, j] = (n + 2) * U * (a64(g).T @ aa) + eg_.T @ aa + a64(g).T @ ee + eg_.T @ ee
    db = np.zeros(cout, dt) if mutant == "missing_bias_gradient" else f(g).sum(0)
    return dW, db, eW, (n + 2) * U * a64(g).sum(0) + eg_.sum(0)


def _pad(s):
    return s // 2 + s % 2


def tconv_fwd(c, w, b, s, lens, slope=SLOPE, ec=None, mutant=None, dt=np.float64):
    """u[s q + p] = b + l(c)[q1] W[:, :, ph] + l(c)[q1 - 1] W[:, :, ph + s], ph = (p + padding) % s, q1 = q + (p + padding) // s -> (u, e_u)"""
    f = lambda v: np.asarray(v, dtype=dt)
    cin, cout = w.shape[0], w.shape[1]
    a, across = lrelu(f(c), slope), mutant == "tconv_across_edge"
    u, eu = np.zeros((len(c) * s, cout), dt), np.zeros((len(c) * s, cout))
    for p in range(s):
        t = p + _pad(s) + (1 if mutant == "phase_off_by_one" else 0)
        ph, cy = t % s, t // s
        v, av, ein = np.tile(f(b), (len(c), 1)), np.tile(a64(b), (len(c), 1)), np.zeros((len(c), cout))
        for sh, kk in ((cy, ph), (cy - 1, ph + s)):
            v = v + shift(a, lens, sh, across) @ f(w[:, :, kk])
            av += shift(a64(a), lens, sh) @ a64(w[:, :, kk])
            if ec is not None:
                ein += shift(ec, lens, sh) @ a64(w[:, :, kk])
        u[p::s], eu[p::s] = v, (2 * cin + 2) * U * av + ein
    return u, eu


def _tap_rows(du, lens, s, j):
    """rows q -> du[s q + j - padding], zero outside the utterance's own output rows"""
    o = j - _pad(s)
    return shift(du[o % s :: s], lens, o // s)


def tconv_dx(c, w, s, lens, du, slope=SLOPE, ec=None, edu=None, mutant=None, dt=np.float64):
    """dc[q] = m(c[q]) * sum_j du[s q + j - padding] W[:, :, j]^T -> (dc, e_dc, unsure)"""
    f = lambda v: np.asarray(v, dtype=dt)
    cin, cout = w.shape[0], w.shape[1]
    S, aS, eS = np.zeros((len(c), cin), dt), np.zeros((len(c), cin)), np.zeros((len(c), cin))
    for j in range(2 * s):
        Wj = w[:, :, j].T
        S = S + _tap_rows(f(du), lens, s, j) @ f(Wj)
        aS += _tap_rows(a64(du), lens, s, j) @ a64(Wj)
        if edu is not None:
            eS += _tap_rows(edu, lens, s, j) @ a64(Wj)
    eS = (2 * s * cout + 1) * U * aS + eS
    return masked(S, aS, eS, c, slope, None, ec, None, mutant, dt)


def tconv_dw(c, s, lens, du, slope=SLOPE, ec=None, edu=None, mutant=None, dt=np.float64):
    """dW[:, :, j] = sum_q l(c)[q]^T du[s q + j - padding], db = sum over the output rows of du -> (dW (cin, cout, 2 s), db, e_dW, e_db)"""
    f = lambda v: np.asarray(v, dtype=dt)
    n, cin, cout = len(c), c.shape[1], du.shape[1]
    a, ea, edu_ = lrelu(f(c), slope), _z(ec, c), _z(edu, du)
    dW, eW = np.zeros((cin, cout, 2 * s), dt), np.zeros((cin, cout, 2 * s))
    for j in range(2 * s):
        g, ag, eg = _tap_rows(f(du), lens, s, j), _tap_rows(a64(du), lens, s, j), _tap_rows(edu_, lens, s, j)
        dW[:, :, j] = a.T @ g
        eW[:, :, j] = (n + 2) * U * (a64(a).T @ ag) + ea.T @ ag + a64(a).T @ eg + ea.T @ eg
    db = np.zeros(cout, dt) if mutant == "missing_bias_gradient" else f(du).sum(0)
    return dW, db, eW, (n * s + 2) * U * a64(du).sum(0) + edu_.sum(0)


def unit_fwd(x, w1, b1, w2, b2, dil, lens, slope=SLOPE, ex=None, mutant=None, dt=np.float64):
    """-> dict xt, e_xt, xo = x' and e_xo"""
    xt, e_xt = conv_fwd(x, w1, b1, dil, lens, slope, ex=ex, dt=dt)
    xo, e_xo = conv_fwd(xt, w2, b2, dil if mutant == "conv2_dilated" else 1, lens, slope, res=x, ex=e_xt, eres=ex, dt=dt)
    return dict(xt=xt, e_xt=e_xt, xo=xo, e_xo=e_xo)


def unit_bwd(x, xt, w1, w2, dil, lens, g, slope=SLOPE, ex=None, ext=None, eg=None, mutant=None, dt=np.float64):
    """on the pre-activations x, xt and g = dx' -> dict dxt, dx, the four parameter gradients dw2, db2, dw1, db1, their bounds e_*, and unsure (the
    larger share of unsure mask cells of xt and x)"""
    k = w1.shape[2]
    dw2, db2, e_dw2, e_db2 = conv_dw(xt, g, k, 1, lens, slope, ex=ext, eg=eg, mutant=mutant, dt=dt)
    dxt, e_dxt, u1 = conv_dx(g, w2, 1, lens, slope, pre=xt, eg=eg, epre=ext, mutant=mutant, dt=dt)
    dw1, db1, e_dw1, e_db1 = conv_dw(x, dxt, k, dil, lens, slope, ex=ex, eg=e_dxt, mutant=mutant, dt=dt)
    dx, e_dx, u2 = conv_dx(dxt, w1, dil, lens, slope, pre=x, carry=g, eg=e_dxt, epre=ex, ecarry=eg, mutant=mutant, dt=dt)
    return dict(dxt=dxt, e_dxt=e_dxt, dx=dx, e_dx=e_dx, grads=[dw1, db1, dw2, db2], e_grads=[e_dw1, e_db1, e_dw2, e_db2], unsure=max(u1, u2))


# ---- a stage and the generator up to the last stage's output ------------------------------------------------------------------------------------
def stage_weights(sd, cfg, i):
    """(wt, bt, per block per unit (w1, b1, w2, b2)) of stage i from a plain state dict, float64"""
    nk, g = len(cfg["resblock_kernel_sizes"]), lambda k: np.asarray(sd[k], dtype=np.float64)
    blocks = []
    for j in range(nk):
        p = "blocks.%d." % (i * nk + j)
        blocks.append([(g(p + "convs1.%d.1.weight" % d), g(p + "convs1.%d.1.bias" % d), g(p + "convs2.%d.1.weight" % d), g(p + "convs2.%d.1.bias" % d))
                       for d in range(len(cfg["resblock_dilations"][j]))])
    return g("upsamples.%d.1.weight" % i), g("upsamples.%d.1.bias" % i), blocks


def stage_fwd(c, W, cfg, i, lens, slope=SLOPE, ec=None, mutant=None, dt=np.float64):
    """c [rows in, cin] with lens at the input rate -> dict u, e_u, units[j][d] (unit_fwd's), out, e_out"""
    wt, bt, blocks = W
    s, nk = cfg["upsample_scales"][i], len(blocks)
    lo = [n * s for n in lens]
    u, e_u = tconv_fwd(c, wt, bt, s, lens, slope, ec, mutant, dt)
    units, tot, atot, etot = [], 0, 0, 0
    for j, blk in enumerate(blocks):
        x, ex, row = u, e_u, []
        for d, (w1, b1, w2, b2) in enumerate(blk):
            r = unit_fwd(x, w1, b1, w2, b2, cfg["resblock_dilations"][j][d], lo, slope, ex, mutant, dt)
            row.append(r)
            x, ex = r["xo"], r["e_xo"]
        units.append(row)
        tot, atot, etot = tot + x, atot + a64(x), etot + ex
    out = tot * dt(1.0 / nk)
    return dict(u=u, e_u=e_u, units=units, out=out, e_out=etot / nk + (nk + 2) * U * atot / nk)


def stage_bwd(c, fw, W, cfg, i, lens, dout, slope=SLOPE, ec=None, edout=None, exact_kept=False, mutant=None, dt=np.float64):
    """fw: the kept pre-activations in stage_fwd's form (with their bounds unless exact_kept: the device's own) -> dict dc, e_dc, grads / e_grads
    ([dwt, dbt] then (dw1, db1, dw2, db2) per block and unit, torch's orientation), du, e_du, unsure (the largest share over the masks)"""
    wt, bt, blocks = W
    s, nk = cfg["upsample_scales"][i], len(blocks)
    lo = [n * s for n in lens]
    e = (lambda v: None) if exact_kept else (lambda v: v)
    seed = np.asarray(dout, dt) * dt(1.0 if mutant == "no_seed_scale" else 1.0 / nk)
    e_seed = _z(edout, dout) / nk + 2 * U * a64(dout) / nk
    du, adu, e_du, grads, e_grads, unsure = 0, 0, 0, [], [], 0.0
    for j, blk in enumerate(blocks):
        g, eg, gj, egj = seed, e_seed, [], []
        for d in range(len(blk) - 1, -1, -1):
            w1, _, w2, _ = blk[d]
            x, ex = (fw["u"], e(fw["e_u"])) if d == 0 else (fw["units"][j][d - 1]["xo"], e(fw["units"][j][d - 1]["e_xo"]))
            r = unit_bwd(x, fw["units"][j][d]["xt"], w1, w2, cfg["resblock_dilations"][j][d], lo, g, slope, ex, e(fw["units"][j][d]["e_xt"]), eg, mutant, dt)
            gj, egj = r["grads"] + gj, r["e_grads"] + egj
            g, eg, unsure = r["dx"], r["e_dx"], max(unsure, r["unsure"])
        grads, e_grads = grads + gj, e_grads + egj
        du, adu, e_du = du + g, adu + a64(g), e_du + eg
    e_du = e_du + nk * U * adu
    dwt, dbt, e_dwt, e_dbt = tconv_dw(c, s, lens, du, slope, ec, e_du, mutant, dt)
    dc, e_dc, uc = tconv_dx(c, wt, s, lens, du, slope, ec, e_du, mutant, dt)
    return dict(dc=dc, e_dc=e_dc, du=du, e_du=e_du, grads=[dwt, dbt] + grads, e_grads=[e_dwt, e_dbt] + e_grads, unsure=max(unsure, uc))


def generator_fwd(sd, cfg, mel, lens, slope=SLOPE, mutant=None, dt=np.float64):
    """input_conv and every stage on the packed mel [frames, in] -> dict c0, e_c0, stages (stage_fwd's), out, e_out (the last stage's output)"""
    g = lambda k: np.asarray(sd[k], dtype=np.float64)
    c0, e_c0 = conv_fwd(mel, g("input_conv.weight"), g("input_conv.bias"), 1, lens, slope, act=False, dt=dt)
    c, ec, ln, stages = c0, e_c0, list(lens), []
    for i, s in enumerate(cfg["upsample_scales"]):
        st = stage_fwd(c, stage_weights(sd, cfg, i), cfg, i, ln, slope, ec, mutant, dt)
        stages.append(st)
        c, ec, ln = st["out"], st["e_out"], [n * s for n in ln]
    return dict(c0=c0, e_c0=e_c0, stages=stages, out=c, e_out=ec)


def generator_bwd(sd, cfg, mel, lens, fw, dout, slope=SLOPE, mutant=None, dt=np.float64):
    """the gradient dout of the last stage's output back to every stage parameter, input_conv's parameters and the mel -> dict grads {state-dict name:
    gradient}, e_grads, dmel, e_dmel, unsure"""
    nk = len(cfg["resblock_kernel_sizes"])
    rates = [1]
    for s in cfg["upsample_scales"]:
        rates.append(rates[-1] * s)
    g, eg, grads, e_grads, unsure = dout, None, {}, {}, 0.0
    for i in range(len(cfg["upsample_scales"]) - 1, -1, -1):
        c, ec = (fw["c0"], fw["e_c0"]) if i == 0 else (fw["stages"][i - 1]["out"], fw["stages"][i - 1]["e_out"])
        r = stage_bwd(c, fw["stages"][i], stage_weights(sd, cfg, i), cfg, i, [n * rates[i] for n in lens], g, slope, ec, eg, False, mutant, dt)
        names = ["upsamples.%d.1.weight" % i, "upsamples.%d.1.bias" % i]
        for j in range(nk):
            for d in range(len(cfg["resblock_dilations"][j])):
                p = "blocks.%d." % (i * nk + j)
                names += [p + "convs1.%d.1.weight" % d, p + "convs1.%d.1.bias" % d, p + "convs2.%d.1.weight" % d, p + "convs2.%d.1.bias" % d]
        grads.update(zip(names, r["grads"]))
        e_grads.update(zip(names, r["e_grads"]))
        g, eg, unsure = r["dc"], r["e_dc"], max(unsure, r["unsure"])
    k = cfg["kernel_size"]
    dw, db, e_dw, e_db = conv_dw(mel, g, k, 1, lens, slope, act=False, eg=eg, mutant=mutant, dt=dt)
    grads["input_conv.weight"], grads["input_conv.bias"], e_grads["input_conv.weight"], e_grads["input_conv.bias"] = dw, db, e_dw, e_db
    dmel, e_dmel, _ = conv_dx(g, np.asarray(sd["input_conv.weight"], np.float64), 1, lens, slope, eg=eg, mutant=mutant, dt=dt)
    return dict(grads=grads, e_grads=e_grads, dmel=dmel, e_dmel=e_dmel, unsure=unsure)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------------
def small_case():
    """(state dict at GAIN, packed mel [sum GENERATOR_LENS, 80], dout [rows of the last stage, its width]) float32"""
    sd, mels = H.generator_inputs(H.SEEDS["small"], H.GENERATOR_LENS, SMALL)
    sd = {k: (v * np.float32(GAIN) if k.endswith("weight") else v) for k, v in sd.items()}
    mel = np.concatenate(mels)
    hop = int(np.prod(SMALL["upsample_scales"]))
    rng = np.random.RandomState(H.SEEDS["small"] + 77)
    dout = rng.standard_normal((len(mel) * hop, SMALL["channels"] >> len(SMALL["upsample_scales"]))).astype(np.float32)
    return sd, mel, dout


def conv_case(k, d, cin, cout=None):
    """(x, w (cout, cin, k), b, res, g) float32 on LENS: hifigan_ref.unit_case's arrays (x, w1, b1, cs0 as the residual / carry and the gradient)"""
    if cout is None:
        x, w1, b1, w2, b2, cs0 = H.unit_case(H.SEEDS["unit"], k, d, cin, list(LENS))
        return x, w1, b1, cs0, (cs0[::-1] * np.float32(0.5)).copy()
    rng = np.random.RandomState(H.SEEDS["unit"] + cin + cout)
    f = lambda *shp: rng.standard_normal(shp).astype(np.float32)
    return f(sum(LENS), cin), f(cout, cin, k) / np.float32(math.sqrt(cin * k)), np.float32(0.5) * f(cout), f(sum(LENS), cout), f(sum(LENS), cout)


def share(diff, bound):
    return float(np.max(np.abs(diff) / np.maximum(bound, 1e-300)))
