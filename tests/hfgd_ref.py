"""The HiFi-GAN period and multi-period discriminators (include/fcl_hip.h "HiFi-GAN period discriminator") stated in float64 numpy: the
per-layer forward, the strided adjoint, the weight and bias gradients, one period end to end (reflection pad, phase-major packing, the direct feature-map
gradients `extra`), the multi-period discriminator with its three losses, and running error bounds for an exact-fp32 evaluation, computed from the
reference alone.  No package code.  A second statement at the end uses torch.nn.functional.conv2d on the [B, 1, H, p] view, F.pad(reflect) and autograd.

The network for period p: x [T] is reflection-padded on the right to a multiple of p and viewed as [H0, p]; segment q is x_pad[h p + q].  Layer l is a
convolution along each segment with k0 taps, stride s_l, padding (k0 - 1) / 2, then LeakyReLU(slope); the score layer has k1 - 1 taps, stride 1, padding
(k1 - 1) / 2 and no activation.  H_out = (H + 2 pad - taps) / stride + 1.  An utterance's activations are held as [p, H, C] (all its segments have the
same height); reshaped to [p H, C] that is its part of the packed, phase-major device layout.  Weights are [cout, cin, taps] (torch's Conv2d without
the trailing 1).

Bounds (u = 2^-24; worst case, so nothing is added to them):
  forward, per cell:   e_l = (k cin + 2 + w_ulps) u (sum |w| |h_{l-1}| + |b|) + sum |w| e_{l-1},  e_{-1} = 0; LeakyReLU is 1-Lipschitz.
  input gradient:      S = sum_taps W^T g + extra, y = m S:  e_S = (k cout + 2 + w_ulps) u (sum |w| |g| + |extra|) + sum |w| eg + e_extra, eg_below = m e_S.
                       On GIVEN activations the mask is a function of the inputs.  End to end the device's mask comes from its own activation: a cell
                       whose float64 pre-activation lies within its own forward bound (an UNSURE cell) may take the other branch and is charged the whole
                       jump: eg_below = e_S + (1 - slope) (|S| + e_S).  At most CAP of an array's cells may be unsure.
  weight gradients:    (rows + 2) u sum_t |g| |h| + sum_t eg |h| (+ sum_t (|g| + eg) eh end to end); the bias gradient likewise with h = 1.
  L1 feature matching: d / d fake = c sign(fake - real), c = weight / cells; a cell with |fake - real| within the sum of the two bounds is unsure as
                       well and is charged the whole jump 2 c; the others 8 u c for the device's float32 evaluation of c."""
import numpy as np

U = 2.0 ** -24
CAP = 0.01
LENS = (11, 130, 1100, 77, 401)
PERIODS = (2, 3, 5, 7, 11)
SMALL = dict(channels=16, max_downsample_channels=64, kernel_sizes=(5, 3), downsample_scales=(3, 3, 3, 3, 1), negative_slope=0.1, bias=True)
GAIN = 0.25  # of the Kaiming scale, for every chained case (see the module docstring of test_hifigan_discriminator_cpu.py for the shares it gives)
MUTANTS = ("stride_plus_one", "across_boundary", "no_divisibility", "taps_not_reversed", "time_major", "zero_pad", "extra_after_mask", "score_three_taps",
           "no_bias_gradient", "slope_one_at_zero")


def out_rows(h, k, s, pad):
    return (h + 2 * pad - k) // s + 1


def geometry(cfg, mutant=None):
    """[(cin, cout, taps, stride, pad)] per layer, the score layer last"""
    k0, k1 = cfg["kernel_sizes"]
    geo, ci, co = [], 1, cfg["channels"]
    for i, s in enumerate(cfg["downsample_scales"]):
        geo.append((ci, co, k0, s + 1 if mutant == "stride_plus_one" and i == 1 else s, (k0 - 1) // 2))
        ci, co = co, min(4 * co, cfg["max_downsample_channels"])
    return geo + [(ci, 1, k1 if mutant == "score_three_taps" else k1 - 1, 1, (k1 - 1) // 2)]


def f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def weights(cfg, seed, gain=GAIN):
    """per layer (W [cout, cin, taps], b [cout] or None): float32 values held in float64; N(0, gain^2 2 / fan_in) weights, N(0, 0.02^2) biases"""
    rng = np.random.default_rng(1000 + seed)
    out = []
    for ci, co, k, _, _ in geometry(cfg):
        W = f32(rng.standard_normal((co, ci, k)) * gain * np.sqrt(2.0 / (ci * k)))
        out.append((W, f32(0.02 * rng.standard_normal(co)) if cfg["bias"] else None))
    return out


def signals(lens, seed):
    """one float32 waveform per utterance (held in float64), N(0, 0.3^2)"""
    rng = np.random.default_rng(2000 + seed)
    return [f32(0.3 * rng.standard_normal(n)) for n in lens]


def normal(shape, seed, scale=1.0):
    return f32(scale * np.random.default_rng(3000 + seed).standard_normal(shape))


# ---- the fold: reflection pad and phase-major segments ----------------------------------------------------------------------------------------------

def fold(x, p, mutant=None):
    """x [T] -> [p, H0, 1]: segment q holds x_pad[h p + q]"""
    T = len(x)
    n_pad = (p - T % p) % p
    assert n_pad < T
    tail = np.zeros(n_pad) if mutant == "zero_pad" else x[T - 2 - np.arange(n_pad)]
    xp = np.concatenate([x, tail])
    seg = xp.reshape(p, -1) if mutant == "time_major" else xp.reshape(-1, p).T
    return np.ascontiguousarray(seg)[:, :, None]


def unfold_adjoint(g, T, p, mutant=None):
    """the adjoint of fold: g [p, H0, 1] -> [T]; a reflected sample's gradient is added to its source"""
    gp = g[:, :, 0].reshape(-1) if mutant == "time_major" else g[:, :, 0].T.reshape(-1)
    out = gp[:T].copy()
    if mutant != "zero_pad":
        i = np.arange(len(gp) - T)
        np.add.at(out, T - 2 - i, gp[T + i])
    return out


# ---- one layer on an utterance's segments [p, H, C] -----------------------------------------------------------------------------------------------------

def _taps(H, k, s, pad):
    """(j, the output rows o whose tap j falls inside [0, H), the input rows s o + j - pad they read)"""
    o = np.arange(out_rows(H, k, s, pad))
    for j in range(k):
        r = s * o + j - pad
        ok = (r >= 0) & (r < H)
        if ok.any():
            yield j, o[ok], r[ok]


def conv(h, W, b, s, pad, mutant=None):
    """h [p, H, cin] -> [p, H_out, cout] = b + sum_j h[s o + j - pad] W[:, :, j]^T, zero outside the segment (the mutant reads the neighbouring segment)"""
    p, H, _ = h.shape
    k = W.shape[2]
    out = np.zeros((p, out_rows(H, k, s, pad), W.shape[0]), dtype=h.dtype) + (0 if b is None else b)
    if mutant == "across_boundary":
        flat, o = h.reshape(p * H, -1), np.arange(out.shape[1])
        for j in range(k):
            r = np.arange(p)[:, None] * H + (s * o + j - pad)[None, :]
            ok = (r >= 0) & (r < p * H)
            out += (flat[np.clip(r, 0, p * H - 1)] * ok[:, :, None]) @ W[:, :, j].T
        return out
    for j, o, r in _taps(H, k, s, pad):
        out[:, o] += h[:, r] @ W[:, :, j].T
    return out


def conv_dx(g, W, s, pad, H, mutant=None):
    """the adjoint: g [p, H_out, cout] -> [p, H, cin], row s o + j - pad collects g[o] W[:, :, j].  Mutants: the gather form without the divisibility test
    (row h takes g[(h + pad - j) // s] for every tap), the taps not reversed"""
    k = W.shape[2]
    out = np.zeros((g.shape[0], H, W.shape[1]), dtype=g.dtype)
    if mutant == "no_divisibility":
        hh = np.arange(H)
        for j in range(k):
            o = (hh + pad - j) // s
            ok = (o >= 0) & (o < g.shape[1])
            out[:, hh[ok]] += g[:, o[ok]] @ W[:, :, j]
        return out
    for j, o, r in _taps(H, k, s, pad):
        out[:, r] += g[:, o] @ W[:, :, k - 1 - j if mutant == "taps_not_reversed" else j]
    return out


def conv_dw(g, h, k, s, pad):
    """-> [cout, cin, k]: sum over segments and rows of g[o, co] h[s o + j - pad, ci]"""
    out = np.zeros((g.shape[2], h.shape[2], k), dtype=g.dtype)
    for j, o, r in _taps(h.shape[1], k, s, pad):
        out[:, :, j] = np.tensordot(g[:, o], h[:, r], axes=([0, 1], [0, 1]))
    return out


def leaky(v, slope):
    return np.where(v > 0, v, slope * v)


def layer_forward(W, b, hin, s, pad, slope, act=True):
    """one layer on a GIVEN input [p, H, cin] -> (output, its bound): the first term of the recursion alone"""
    pre = conv(hin, W, b, s, pad)
    e = (W.shape[2] * W.shape[1] + 2) * U * conv(np.abs(hin), np.abs(W), None if b is None else np.abs(b), s, pad)
    return (leaky(pre, slope) if act else pre), e


def layer_dx(W, g, hin, extra, s, pad, slope, mask=True, mutant=None):
    """one layer's input gradient on GIVEN g [p, H_out, cout], hin [p, H, cin] (the stored activation of its input) and extra (or None) -> (y, its bound)"""
    H = hin.shape[1]
    S = conv_dx(g, W, s, pad, H, mutant)
    eS = (W.shape[2] * W.shape[0] + 2) * U * (conv_dx(np.abs(g), np.abs(W), s, pad, H) + (0.0 if extra is None else np.abs(extra)))
    m = np.where(hin >= 0 if mutant == "slope_one_at_zero" else hin > 0, 1.0, slope) if mask else 1.0
    if extra is not None:
        return (m * S + extra, m * eS) if mutant == "extra_after_mask" else (m * (S + extra), m * eS)
    return m * S, m * eS


def layer_dw(g, hin, k, s, pad, rows):
    """(dw, its bound, db, its bound) on GIVEN g and hin of one utterance; rows: the output rows of the whole batch (the length of the device's sum)"""
    return (conv_dw(g, hin, k, s, pad), (rows + 2) * U * conv_dw(np.abs(g), np.abs(hin), k, s, pad), g.sum((0, 1)), (rows + 2) * U * np.abs(g).sum((0, 1)))


# ---- one period end to end ----------------------------------------------------------------------------------------------------------------------------

def forward(cfg, ws, xs, p, mutant=None, w_ulps=0):
    """per utterance dict(x [p, H0, 1], pre, h, e per layer [p, H_l, C_l]; the last layer's h = pre = the scores [p, H', 1])"""
    geo, slope = geometry(cfg, mutant), cfg["negative_slope"]
    out = []
    for x in xs:
        h = fold(x, p, mutant)
        r = dict(x=h, pre=[], h=[], e=[])
        e = np.zeros_like(h)
        for l, ((W, b), (ci, co, k, s, pad)) in enumerate(zip(ws, geo)):
            if mutant == "score_three_taps" and l == len(geo) - 1:
                W = np.concatenate([W, W[:, :, :1]], 2)
            pre = conv(h, W, b, s, pad, mutant)
            e = (k * ci + 2 + w_ulps) * U * conv(np.abs(h), np.abs(W), None if b is None else np.abs(b), s, pad) + conv(e, np.abs(W), None, s, pad)
            h = leaky(pre, slope) if l < len(geo) - 1 else pre
            r["pre"].append(pre), r["h"].append(h), r["e"].append(e)
        out.append(r)
    return out


def unsure_cells(fw):
    """per layer with an activation: per utterance the cells whose pre-activation lies within its own bound"""
    L = len(fw[0]["pre"]) - 1
    return [[np.abs(r["pre"][l]) <= r["e"][l] for r in fw] for l in range(L)]


def unsure_shares(fw):
    """the share of unsure cells per layer's array (the whole batch)"""
    return [sum(int(a.sum()) for a in layer) / sum(a.size for a in layer) for layer in unsure_cells(fw)]


def backward(cfg, ws, fw, dscores, extras=None, mutant=None, end_to_end=False, eg_in=None, e_extras=None, w_ulps=0):
    """fw: forward()'s result (its x and h are the stored activations); dscores [utt] [p, H', 1]; extras [utt][l] [p, H_l, C_l] or None: the direct gradient
    of map l -> dict(gx, gx_e per utterance [p, H0, 1] (period_backward unfolds them to [T]); dw, dw_e, db, db_e per layer, summed over the batch).  end_to_end: the activations
    carry their forward bounds and the unsure cells their jump; eg_in [utt]: the bound the given dscore already carries; e_extras [utt][l]: that of extra."""
    geo, slope = geometry(cfg, mutant), cfg["negative_slope"]
    L = len(geo)
    rows = [sum(r["h"][l].shape[0] * r["h"][l].shape[1] for r in fw) for l in range(L)]
    z = lambda: [np.zeros(W.shape, dtype=W.dtype) for W, _ in ws]
    zb = lambda: [np.zeros(W.shape[0], dtype=W.dtype) for W, _ in ws]
    out = dict(gx=[], gx_e=[], dw=z(), dw_e=z(), db=zb(), db_e=zb(), g_peak=[0.0] * L, g_bound=[0.0] * L)
    for u, r in enumerate(fw):
        g = dscores[u]
        eg = np.zeros_like(g) if eg_in is None else eg_in[u]
        for l in range(L - 1, -1, -1):
            (W, _), (ci, co, k, s, pad) = ws[l], geo[l]
            below = r["x"] if l == 0 else r["h"][l - 1]
            out["g_peak"][l], out["g_bound"][l] = max(out["g_peak"][l], np.abs(g).max()), max(out["g_bound"][l], eg.max())
            out["dw"][l] += conv_dw(g, below, k, s, pad)
            out["dw_e"][l] += (rows[l] + 2) * U * conv_dw(np.abs(g), np.abs(below), k, s, pad) + conv_dw(eg, np.abs(below), k, s, pad)
            if end_to_end and l > 0:
                out["dw_e"][l] += conv_dw(np.abs(g) + eg, r["e"][l - 1], k, s, pad)
            if mutant != "no_bias_gradient":
                out["db"][l] += g.sum((0, 1))
            out["db_e"][l] += (rows[l] + 2) * U * np.abs(g).sum((0, 1)) + eg.sum((0, 1))
            H = below.shape[1]
            ex = None if (extras is None or l == 0 or extras[u][l - 1] is None) else extras[u][l - 1]
            S = conv_dx(g, W, s, pad, H, mutant)
            eS = (k * co + 2 + w_ulps) * U * (conv_dx(np.abs(g), np.abs(W), s, pad, H) + (0.0 if ex is None else np.abs(ex))) + conv_dx(eg, np.abs(W), s, pad, H)
            if ex is not None and e_extras is not None:
                eS = eS + e_extras[u][l - 1]
            if l == 0:
                out["gx"].append(S), out["gx_e"].append(eS)
                continue
            m = np.where(below >= 0 if mutant == "slope_one_at_zero" else below > 0, 1.0, slope).astype(below.dtype)
            if ex is not None:
                g = m * S + ex if mutant == "extra_after_mask" else m * (S + ex)
                S = S + ex
            else:
                g = m * S
            eg = m * eS
            if end_to_end:
                unsure = np.abs(r["pre"][l - 1]) <= r["e"][l - 1]
                eg = np.where(unsure, eS + (1.0 - slope) * (np.abs(S) + eS), eg)
    return out


def period_backward(cfg, ws, xs, fw, dscores, p, **kw):
    """backward() with the waveform gradients unfolded to [T] per utterance"""
    out = backward(cfg, ws, fw, dscores, **kw)
    mutant = kw.get("mutant")
    out["gx"] = [unfold_adjoint(g, len(x), p, mutant) for g, x in zip(out["gx"], xs)]
    out["gx_e"] = [unfold_adjoint(e, len(x), p) for e, x in zip(out["gx_e"], xs)]
    return out


def pack(arrs):
    """per-utterance [p, H, C] arrays -> the device's packed [rows, C]"""
    return np.concatenate([a.reshape(-1, a.shape[2]) for a in arrs])


def unpack(a, like):
    """the device's packed [rows, C] (or [rows]) -> per-utterance arrays shaped as `like`"""
    a = a.reshape(-1, like[0].shape[2])
    cuts = np.cumsum([v.shape[0] * v.shape[1] for v in like])[:-1]
    return [part.reshape(v.shape) for part, v in zip(np.split(a, cuts), like)]


def given_gradients(fw, seed, with_extras=True):
    """a float32 dscore per utterance and, per map, a direct gradient (map 1 gets none: an absent gradient among present ones)"""
    ds, ex = [], []
    for u, r in enumerate(fw):
        ds.append(normal(r["h"][-1].shape, 100 * seed + u))
        ex.append([None if (l == 1 or not with_extras) else normal(h.shape, 100 * seed + 10 * l + u + 50, 0.05) for l, h in enumerate(r["h"][:-1])])
    return ds, ex


# ---- weight norm ------------------------------------------------------------------------------------------------------------------------------------------

def fold_weight(v, g):
    """w = v g / ||v|| over every dim but 0"""
    return v * (g / np.sqrt((v ** 2).sum((1, 2))))[:, None, None]


def weight_norm_gradients(v, g, dw):
    """-> (dg [cout], dv) from dw"""
    nrm = np.sqrt((v ** 2).sum((1, 2)))
    dot = (dw * v).sum((1, 2))
    return dot / nrm, (g / nrm)[:, None, None] * dw - (g * dot / nrm ** 3)[:, None, None] * v


# ---- the multi-period discriminator with its three losses -------------------------------------------------------------------------------------------------

def mse(scores, target):
    """mean (p - target)^2 over every score cell of a batch"""
    return sum(((s - target) ** 2).sum() for s in scores) / sum(s.size for s in scores)


def mse_bound(scores, es, target):
    return sum((2 * np.abs(s - target) * e + e ** 2).sum() for s, e in zip(scores, es)) / sum(s.size for s in scores) + 8 * U * mse(scores, target)


def mpd_reference(cfg, wss, real, fake, periods=PERIODS, w_adv=1.0, w_fm=2.0):
    """wss: the weights per period.  -> dict(adv, fm, d_real, d_fake with their bounds *_e; gx, gx_e per fake utterance: the gradient of
    w_adv adv + w_fm fm to the fake waveform; unsure: the worst share of unsure cells of any array, mask and L1 cells together)"""
    P = len(periods)
    out = dict(adv=0.0, adv_e=0.0, fm=0.0, fm_e=0.0, d_real=0.0, d_real_e=0.0, d_fake=0.0, d_fake_e=0.0, unsure=0.0)
    gx, gx_e = [np.zeros(len(x)) for x in fake], [np.zeros(len(x)) for x in fake]
    for ws, p in zip(wss, periods):
        fr, ff = forward(cfg, ws, real, p), forward(cfg, ws, fake, p)
        L = len(ws) - 1
        sc_r, sc_f = [r["h"][-1] for r in fr], [r["h"][-1] for r in ff]
        e_r, e_f = [r["e"][-1] for r in fr], [r["e"][-1] for r in ff]
        out["adv"] += mse(sc_f, 1.0) / P
        out["adv_e"] += mse_bound(sc_f, e_f, 1.0) / P
        out["d_real"] += mse(sc_r, 1.0) / P
        out["d_real_e"] += mse_bound(sc_r, e_r, 1.0) / P
        out["d_fake"] += mse(sc_f, 0.0) / P
        out["d_fake_e"] += mse_bound(sc_f, e_f, 0.0) / P
        n_sc = sum(s.size for s in sc_f)
        ds = [w_adv * 2.0 * (s - 1.0) / (n_sc * P) for s in sc_f]
        eg = [w_adv * 2.0 * e / (n_sc * P) + 8 * U * np.abs(d) for e, d in zip(e_f, ds)]
        extras, e_extras = [[] for _ in fake], [[] for _ in fake]
        mask_unsure = unsure_cells(ff)
        for l in range(L):
            cells = sum(r["h"][l].size for r in ff)
            c = w_fm / (cells * L * P)
            kinks = 0
            for u in range(len(fake)):
                d, tol = ff[u]["h"][l] - fr[u]["h"][l], ff[u]["e"][l] + fr[u]["e"][l]
                near = np.abs(d) <= tol
                kinks += int((near | mask_unsure[l][u]).sum())
                extras[u].append(c * np.sign(d))
                e_extras[u].append(np.where(near, 2 * c, 8 * U * c))
                out["fm"] += np.abs(d).sum() / (cells * L * P)
                out["fm_e"] += tol.sum() / (cells * L * P) + 8 * U * np.abs(d).sum() / (cells * L * P)
            out["unsure"] = max(out["unsure"], kinks / cells)
        bw = period_backward(cfg, ws, fake, ff, ds, p, extras=extras, end_to_end=True, eg_in=eg, e_extras=e_extras)
        for u in range(len(fake)):
            gx[u] += bw["gx"][u]
            gx_e[u] += bw["gx_e"][u] + 2 * U * np.abs(gx[u])
    out["gx"], out["gx_e"] = gx, gx_e
    return out


# ---- the second statement: torch.nn.functional.conv2d on the [B, 1, H, p] view, F.pad(reflect) and autograd, float64 on the CPU --------------------------

def torch_statement(cfg, ws, xs, p, dscores=None, extras=None, weight_norm=None):
    """-> dict(h [utt][l] as forward()'s h; with dscores also gx [utt], dw, db per layer).  The loss is sum dscore scores + sum_l sum extra_l map_l, whose
    gradients are those of backward().  weight_norm: per layer (v, g) replacing W (then also dv, dg)."""
    import torch
    import torch.nn.functional as F

    geo = geometry(cfg)
    T64 = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)
    if weight_norm is not None:
        vt, gt = [T64(v[..., None]) for v, _ in weight_norm], [T64(g.reshape(-1, 1, 1, 1)) for _, g in weight_norm]
        Wt = [v * (g / torch.linalg.vector_norm(v, dim=(1, 2, 3), keepdim=True)) for v, g in zip(vt, gt)]
    else:
        Wt = [T64(W[..., None]) for W, _ in ws]
    bt = [None if b is None else T64(b) for _, b in ws]
    to_seg = lambda a: a[0].permute(2, 1, 0)  # [1, C, H, p] -> [p, H, C]
    out, total = dict(h=[], gx=[]), 0.0
    xts = []
    for u, x in enumerate(xs):
        xt = T64(x)
        xts.append(xt)
        h = xt[None, None, :]
        if len(x) % p:
            h = F.pad(h, (0, p - len(x) % p), "reflect")
        h = h.view(1, 1, -1, p)
        hs = []
        for l, (ci, co, k, s, pad) in enumerate(geo):
            h = F.conv2d(h, Wt[l], bt[l], stride=(s, 1), padding=(pad, 0))
            if l < len(geo) - 1:
                h = F.leaky_relu(h, cfg["negative_slope"])
            hs.append(h)
        out["h"].append([to_seg(a).detach().numpy() for a in hs])
        if dscores is not None:
            total = total + (to_seg(hs[-1]) * torch.tensor(dscores[u])).sum()
            for l, ex in enumerate(extras[u] if extras is not None else []):
                if ex is not None:
                    total = total + (to_seg(hs[l]) * torch.tensor(ex)).sum()
    if dscores is not None:
        total.backward()
        out["gx"] = [xt.grad.numpy() for xt in xts]
        out["db"] = [None if b is None else b.grad.numpy() for b in bt]
        if weight_norm is not None:
            out["dv"], out["dg"] = [v.grad.numpy()[..., 0] for v in vt], [g.grad.numpy().reshape(-1) for g in gt]
        else:
            out["dw"] = [w.grad.numpy()[..., 0] for w in Wt]
    return out


def torch_losses(outs_real, outs_fake):
    """the three losses in torch on per-period lists [map_0, .., scores] of float64 tensors: (adv, fm, d_real, d_fake)"""
    import torch

    P = len(outs_fake)
    adv = sum(torch.mean((o[-1] - 1.0) ** 2) for o in outs_fake) / P
    d_real = sum(torch.mean((o[-1] - 1.0) ** 2) for o in outs_real) / P
    d_fake = sum(torch.mean(o[-1] ** 2) for o in outs_fake) / P
    fm = sum(sum(torch.nn.functional.l1_loss(f, r.detach()) for f, r in zip(of[:-1], orl[:-1])) / (len(of) - 1) for of, orl in zip(outs_fake, outs_real)) / P
    return adv, fm, d_real, d_fake


# ---- the cases the CPU and the GPU tests share -------------------------------------------------------------------------------------------------------------

# The L1 term's kink needs |fake - real| above the sum of the two cells' bounds in 99 % of a map's cells.  A worst-case bound grows by sum |w| per layer,
# about sqrt(2 fan_in / pi) times faster than the signal itself (10 x at 16 channels, 20 x at 64), whatever the gain: on SMALL's five layers the last two maps
# have 6 % to 60 % such cells at gain 1/4 and more at 1/8.  The multi-period case therefore runs three layers (16 -> 32 -> 32, scales 3, 3, 1), where the
# worst map stays below the cap; SMALL's depth is covered by period_case, whose direct gradients are given and have no kink.
MPD_CFG = dict(channels=16, max_downsample_channels=32, kernel_sizes=(5, 3), downsample_scales=(3, 3, 1), negative_slope=0.1, bias=True)
MPD_LENS = (130, 401, 77)


def period_case(p, gain=GAIN):
    """one period end to end on SMALL: the inputs, the float64 forward, given gradients for every output, and the float64 backward with its running bounds"""
    ws, xs = weights(SMALL, p, gain), signals(LENS, p)
    fw = forward(SMALL, ws, xs, p)
    ds, ex = given_gradients(fw, p)
    bw = period_backward(SMALL, ws, xs, fw, ds, p, extras=ex, end_to_end=True)
    return dict(cfg=SMALL, p=p, ws=ws, xs=xs, fw=fw, ds=ds, ex=ex, bw=bw)


def mpd_case(gain=GAIN):
    wss = [weights(MPD_CFG, 20 + i, gain) for i in range(len(PERIODS))]
    real, fake = signals(MPD_LENS, 7), signals(MPD_LENS, 8)
    return dict(cfg=MPD_CFG, wss=wss, real=real, fake=fake, ref=mpd_reference(MPD_CFG, wss, real, fake))
