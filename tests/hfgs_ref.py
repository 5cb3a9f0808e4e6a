"""The HiFi-GAN scale, multi-scale and multi-scale + multi-period discriminators (include/fcl_hip.h "HiFi-GAN scale discriminator") stated in
float64 numpy: the grouped strided convolution with its input and weight gradients, the average pooling with its adjoint, the layer stack, spectral norm, the
multi-scale discriminator with the three losses, the combined one (the periods through tests/hfgd_ref.py), and running error bounds for an exact-fp32
evaluation, computed from the reference alone.  No package code.  A second statement at the end uses torch.nn.functional.conv1d(groups=), F.avg_pool1d and
autograd.

The network: layer 0 is Conv1d(1 -> channels, k0); then per downsample scale s a grouped Conv1d(cin -> cout, k1, stride s, groups), starting from
(cin, cout, groups) = (channels, channels, 4) and, after each, cin = cout, cout = min(2 cin, max), groups = min(4 groups, max_groups); then a dense
Conv1d(cin -> min(2 cin, max), k2) and the score layer Conv1d(-> 1, k3); padding (k - 1) / 2, LeakyReLU(slope) after all but the score layer.  Output
channel co belongs to group co // (cout / groups) and reads the input channels [g cin / groups, (g + 1) cin / groups).  An utterance's activations are held
as [1, T_l, C] (hfgd_ref's [p, H, C] with one segment), weights as torch's Conv1d [cout, cin / groups, k].  Scale discriminator i sees the waveform pooled
i times: y[n] = (x[2n - 2] + x[2n - 1] + x[2n] + x[2n + 1]) / 4 for n = 0 .. T // 2, zeros outside the utterance, the pad counted in the divisor.

Bounds (u = 2^-24; worst case, so nothing is added to them), as hfgd_ref's with the group's own contraction length:
  forward, per cell:   e_l = (k cin / groups + 2 + w_ulps) u (sum |w| |h_{l-1}| + |b|) + sum |w| e_{l-1}; e_{-1} = the bound the (pooled) waveform carries.
  input gradient:      S = sum_taps W^T g + extra, y = m S:  e_S = (k cout / groups + 2 + w_ulps) u (sum |w| |g| + |extra|) + sum |w| eg + e_extra; on given
                       activations eg_below = m e_S; end to end an UNSURE cell (float64 pre-activation within its own forward bound) is charged the whole
                       jump: eg_below = e_S + (1 - slope) (|S| + e_S).  At most CAP of an array's cells may be unsure.
  weight gradients:    (rows + 2) u sum_t |g| |h| + sum_t eg |h| (+ sum_t (|g| + eg) eh end to end); the bias gradient likewise with h = 1.
  pooling:             3 u sum |x| / 4 + the pooled carried error; the adjoint likewise.
  L1 feature matching: as hfgd_ref: a cell with |fake - real| within the sum of the two bounds is unsure and is charged 2 c, the others 8 u c.

Chained configurations.  A worst-case bound grows by sum |w| per layer, and 41 taps make that worse than under the period discriminator: the default depth
cannot be chained under the cap.  Re-measured here on lengths (130, 1100, 77, 401, 2500), waveform N(0, 0.3^2), biases N(0, 0.02^2), weights at gain 1/4
of Kaiming, three scales (mask cells, the worst map of any scale; test_hifigan_scale_discriminator_cpu.py prints and asserts them):
  CHAIN_A  channels 128, max 256, max_groups 16, kernel_sizes (5, 11, 3, 3), scales (2, 4): both group shapes (32 / 32 and 8 / 16 channels per group);
           worst map 0.33 % unsure cells.
  CHAIN_B  channels 64, max 128, max_groups 4, kernel_sizes (15, 41, 5, 3), scales (4,): the published tap counts; worst map 0.39 % unsure cells.
With these seeds the worst map has 0.54 % (A) and 0.28 % (B) unsure cells.
The multi-scale case with the L1 term (MSD_CFG) has to give way further: the L1 kink makes a cell unsure where |fake - real| lies within the sum of two
bounds, and on CHAIN_A without its second grouped layer the dense map had 4.5 % to 5.7 % such cells (three scales), at 64 channels with kernel sizes
(5, 11, 3, 3) still 1.0 % to 1.7 %.  The narrowest shape the kernels take -- 64 channels in 4 groups, kernel sizes (5, 3, 3, 3), one grouped layer -- has at
most 0.50 % (mask and L1 cells together, the dense map of scale 2).  The default depth, widths and tap counts are covered by the layer-alone cases of the
GPU test."""
import numpy as np

import hfgd_ref as D

U, CAP, GAIN = D.U, D.CAP, D.GAIN
LENS = (130, 1100, 77, 401, 2500)
CHAIN_A = dict(channels=128, max_downsample_channels=256, max_groups=16, kernel_sizes=(5, 11, 3, 3), downsample_scales=(2, 4), negative_slope=0.1, bias=True)
CHAIN_B = dict(channels=64, max_downsample_channels=128, max_groups=4, kernel_sizes=(15, 41, 5, 3), downsample_scales=(4,), negative_slope=0.1, bias=True)
CHAINS = dict(A=CHAIN_A, B=CHAIN_B)
MSD_CFG = dict(channels=64, max_downsample_channels=64, max_groups=4, kernel_sizes=(5, 3, 3, 3), downsample_scales=(2,), negative_slope=0.1, bias=True)
MSD_LENS = (130, 401, 77)
SMALL_PERIOD = D.MPD_CFG
MUTANTS = ("groups_ignored", "membership_modulo", "pool_divisor_without_pad", "pool_pad_one_side", "pooled_length_floor", "stride_plus_one",
           "across_boundary", "taps_not_reversed", "extra_after_mask", "sigma_before_iteration")

f32, normal, signals, leaky, out_rows, pack, unpack = D.f32, D.normal, D.signals, D.leaky, D.out_rows, D.pack, D.unpack


def geometry(cfg, mutant=None):
    """[(cin, cout, taps, stride, pad, groups)] per layer, the score layer last"""
    k0, k1, k2, k3 = cfg["kernel_sizes"]
    ch, mx = cfg["channels"], cfg["max_downsample_channels"]
    geo = [(1, ch, k0, 1, (k0 - 1) // 2, 1)]
    ci, co, gr = ch, ch, 4
    for i, s in enumerate(cfg["downsample_scales"]):
        geo.append((ci, co, k1, s + 1 if mutant == "stride_plus_one" and i == 0 else s, (k1 - 1) // 2, gr))
        ci, co, gr = co, min(2 * co, mx), min(4 * gr, cfg["max_groups"])
    co = min(2 * ci, mx)
    return geo + [(ci, co, k2, 1, (k2 - 1) // 2, 1), (co, 1, k3, 1, (k3 - 1) // 2, 1)]


def weights(cfg, seed, gain=GAIN):
    """per layer (W [cout, cin / groups, taps], b [cout] or None): float32 values held in float64; N(0, gain^2 2 / fan_in) weights, N(0, 0.02^2) biases"""
    rng = np.random.default_rng(5000 + seed)
    out = []
    for ci, co, k, _, _, gr in geometry(cfg):
        W = f32(rng.standard_normal((co, ci // gr, k)) * gain * np.sqrt(2.0 / (ci // gr * k)))
        out.append((W, f32(0.02 * rng.standard_normal(co)) if cfg["bias"] else None))
    return out


# ---- the grouped convolution on an utterance [1, T, C], group by group through hfgd_ref's dense statement -------------------------------------------------

def _groups(co, ci, groups, mutant=None):
    """per group (its output channels, its input channels)"""
    cog, cig = co // groups, ci // groups
    for g in range(groups):
        cols = np.arange(co)[np.arange(co) % groups == g] if mutant == "membership_modulo" else np.arange(g * cog, (g + 1) * cog)
        yield cols, np.arange(cig) if mutant == "groups_ignored" else np.arange(g * cig, (g + 1) * cig)


def gconv(h, W, b, s, pad, groups, mutant=None):
    """h [1, T, cin] -> [1, T_out, cout]: y[:, co] = b[co] + sum_j h[s o + j - pad, its group's channels] W[co, :, j], zero outside the utterance"""
    co, k = W.shape[0], W.shape[2]
    out = np.zeros((h.shape[0], out_rows(h.shape[1], k, s, pad), co), dtype=np.result_type(h.dtype, W.dtype))
    for cols, chans in _groups(co, h.shape[2], groups, mutant):
        out[:, :, cols] = D.conv(h[:, :, chans], W[cols], None if b is None else b[cols], s, pad)
    return out


def gconv_dx(g, W, s, pad, T, groups, cin, mutant=None):
    """the adjoint: g [1, T_out, cout] -> [1, T, cin]"""
    out = np.zeros((g.shape[0], T, cin), dtype=np.result_type(g.dtype, W.dtype))
    for cols, chans in _groups(W.shape[0], cin, groups, mutant):
        out[:, :, chans] += D.conv_dx(g[:, :, cols], W[cols], s, pad, T, "taps_not_reversed" if mutant == "taps_not_reversed" else None)
    return out


def gconv_dw(g, h, k, s, pad, groups):
    """-> [cout, cin / groups, k]"""
    co, ci = g.shape[2], h.shape[2]
    out = np.zeros((co, ci // groups, k), dtype=np.result_type(g.dtype, h.dtype))
    for cols, chans in _groups(co, ci, groups):
        out[cols] = D.conv_dw(g[:, :, cols], h[:, :, chans], k, s, pad)
    return out


def layer_forward(W, b, hin, s, pad, slope, groups=1, act=True):
    """one layer on a GIVEN input [1, T, cin] -> (output, its bound): the first term of the recursion alone"""
    pre = gconv(hin, W, b, s, pad, groups)
    e = (W.shape[2] * W.shape[1] + 2) * U * gconv(np.abs(hin), np.abs(W), None if b is None else np.abs(b), s, pad, groups)
    return (leaky(pre, slope) if act else pre), e


def layer_dx(W, g, hin, extra, s, pad, slope, groups=1, mask=True, mutant=None):
    """one layer's input gradient on GIVEN g [1, T_out, cout], hin [1, T, cin] and extra (or None) -> (y, its bound)"""
    T, ci = hin.shape[1], hin.shape[2]
    S = gconv_dx(g, W, s, pad, T, groups, ci, mutant)
    eS = (W.shape[2] * (W.shape[0] // groups) + 2) * U * (gconv_dx(np.abs(g), np.abs(W), s, pad, T, groups, ci) + (0.0 if extra is None else np.abs(extra)))
    m = np.where(hin > 0, 1.0, slope) if mask else 1.0
    if extra is not None:
        return (m * S + extra, m * eS) if mutant == "extra_after_mask" else (m * (S + extra), m * eS)
    return m * S, m * eS


def layer_dw(g, hin, k, s, pad, rows, groups=1):
    """(dw, its bound, db, its bound) on GIVEN g and hin of one utterance; rows: the output rows of the whole batch (the length of the device's sum)"""
    return (gconv_dw(g, hin, k, s, pad, groups), (rows + 2) * U * gconv_dw(np.abs(g), np.abs(hin), k, s, pad, groups), g.sum((0, 1)),
            (rows + 2) * U * np.abs(g).sum((0, 1)))


# ---- the pooling --------------------------------------------------------------------------------------------------------------------------------------------

def pooled_length(T, mutant=None):
    return T // 2 if mutant == "pooled_length_floor" else T // 2 + 1


def pool(x, mutant=None):
    """x [T] -> [T // 2 + 1]: y[n] = (x[2n - 2] + x[2n - 1] + x[2n] + x[2n + 1]) / 4, zeros outside, the pad counted in the divisor"""
    T = len(x)
    n = np.arange(pooled_length(T, mutant))
    first = 2 * n if mutant == "pool_pad_one_side" else 2 * n - 2
    out, count = np.zeros(len(n), dtype=x.dtype), np.zeros(len(n))
    for j in range(4):
        r = first + j
        ok = (r >= 0) & (r < T)
        out[ok] += x[r[ok]]
        count += ok
    return out / count if mutant == "pool_divisor_without_pad" else out / 4


def pool_adjoint(g, T):
    """g [T // 2 + 1] -> [T]: dx[m] = (g[m // 2] + g[m // 2 + 1]) / 4, the second term where that output exists"""
    m = np.arange(T)
    n1 = m // 2
    out = g[n1].copy()
    ok = n1 + 1 < len(g)
    out[ok] += g[n1[ok] + 1]
    return out / 4


def pool_bound(x, e):
    """the bound of a float32 pooling of a float32 x that carries the bound e"""
    return 3 * U * pool(np.abs(x)) + pool(e)


def pool_chain(x, times, mutant=None):
    """-> [(x_i, e_i)] for i = 0 .. times: the waveform pooled i times and the bound it carries on the device"""
    out = [(x, np.zeros_like(x))]
    for _ in range(times):
        x, e = out[-1]
        out.append((pool(x, mutant), pool_bound(x, e)))
    return out


# ---- one scale discriminator end to end ------------------------------------------------------------------------------------------------------------------------

def forward(cfg, ws, xs, mutant=None, w_ulps=0, e_in=None):
    """per utterance dict(x [1, T, 1], e_x, pre, h, e per layer [1, T_l, C_l]; the last layer's h = pre = the scores [1, T', 1]); e_in: the bound x carries"""
    geo, slope = geometry(cfg, mutant), cfg["negative_slope"]
    out = []
    for u, x in enumerate(xs):
        h = np.asarray(x)[None, :, None]
        e = np.zeros_like(h) if e_in is None else e_in[u][None, :, None]
        r = dict(x=h, e_x=e, pre=[], h=[], e=[])
        for l, ((W, b), (ci, co, k, s, pad, gr)) in enumerate(zip(ws, geo)):
            if mutant == "across_boundary" and l == 1:
                pre = _across(out, h, W, b, s, pad, gr)
            else:
                pre = gconv(h, W, b, s, pad, gr, mutant)
            e = (k * (ci // gr) + 2 + w_ulps) * U * gconv(np.abs(h), np.abs(W), None if b is None else np.abs(b), s, pad, gr) + gconv(e, np.abs(W), None, s, pad, gr)
            h = leaky(pre, slope) if l < len(geo) - 1 else pre
            r["pre"].append(pre), r["h"].append(h), r["e"].append(e)
        out.append(r)
    return out


def _across(done, h, W, b, s, pad, gr):
    """the mutant that reads the previous utterance's last rows where the left pad should be: the layer on [previous tail | h], its first rows dropped"""
    if not done:
        return gconv(h, W, b, s, pad, gr)
    tail = done[-1]["h"][0][:, -s * pad:]  # a multiple of the stride, so the output rows stay aligned
    both = gconv(np.concatenate([tail, h], 1), W, b, s, pad, gr)
    return both[:, tail.shape[1] // s:][:, : out_rows(h.shape[1], W.shape[2], s, pad)]


def unsure_cells(fw):
    return D.unsure_cells(fw)


def unsure_shares(fw):
    return D.unsure_shares(fw)


def backward(cfg, ws, fw, dscores, extras=None, mutant=None, end_to_end=False, eg_in=None, e_extras=None, w_ulps=0):
    """as hfgd_ref.backward on the grouped layers: fw from forward(); dscores [utt] [1, T', 1]; extras [utt][l] or None -> dict(gx, gx_e per utterance [T];
    dw, dw_e, db, db_e per layer, summed over the batch; g_peak, g_bound per layer)"""
    geo, slope = geometry(cfg, mutant), cfg["negative_slope"]
    L = len(geo)
    rows = [sum(r["h"][l].shape[1] for r in fw) for l in range(L)]
    z = lambda: [np.zeros(W.shape, dtype=W.dtype) for W, _ in ws]
    zb = lambda: [np.zeros(W.shape[0], dtype=W.dtype) for W, _ in ws]
    out = dict(gx=[], gx_e=[], dw=z(), dw_e=z(), db=zb(), db_e=zb(), g_peak=[0.0] * L, g_bound=[0.0] * L)
    for u, r in enumerate(fw):
        g = dscores[u]
        eg = np.zeros_like(g) if eg_in is None else eg_in[u]
        for l in range(L - 1, -1, -1):
            (W, _), (ci, co, k, s, pad, gr) = ws[l], geo[l]
            below, e_below = (r["x"], r["e_x"]) if l == 0 else (r["h"][l - 1], r["e"][l - 1])
            out["g_peak"][l], out["g_bound"][l] = max(out["g_peak"][l], np.abs(g).max()), max(out["g_bound"][l], eg.max())
            out["dw"][l] += gconv_dw(g, below, k, s, pad, gr)
            out["dw_e"][l] += (rows[l] + 2) * U * gconv_dw(np.abs(g), np.abs(below), k, s, pad, gr) + gconv_dw(eg, np.abs(below), k, s, pad, gr)
            if end_to_end:
                out["dw_e"][l] += gconv_dw(np.abs(g) + eg, e_below, k, s, pad, gr)
            out["db"][l] += g.sum((0, 1))
            out["db_e"][l] += (rows[l] + 2) * U * np.abs(g).sum((0, 1)) + eg.sum((0, 1))
            T = below.shape[1]
            ex = None if (extras is None or l == 0 or extras[u][l - 1] is None) else extras[u][l - 1]
            S = gconv_dx(g, W, s, pad, T, gr, ci, mutant)
            eS = (k * (co // gr) + 2 + w_ulps) * U * (gconv_dx(np.abs(g), np.abs(W), s, pad, T, gr, ci) + (0.0 if ex is None else np.abs(ex))) + gconv_dx(
                eg, np.abs(W), s, pad, T, gr, ci)
            if ex is not None and e_extras is not None:
                eS = eS + e_extras[u][l - 1]
            if l == 0:
                out["gx"].append(S[0, :, 0]), out["gx_e"].append(eS[0, :, 0])
                continue
            m = np.where(below > 0, 1.0, slope).astype(below.dtype)
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


def given_gradients(fw, seed, with_extras=True):
    """a float32 dscore per utterance and, per map, a direct gradient (map 1 gets none: an absent gradient among present ones)"""
    return D.given_gradients(fw, seed, with_extras)


# ---- spectral norm ---------------------------------------------------------------------------------------------------------------------------------------------

EPS = 1e-12


def spectral_iterate(W, u, v):
    """one power iteration on the [cout, -1] matrix: v = normalize(W^T u), u = normalize(W v)"""
    M = W.reshape(W.shape[0], -1)
    v = M.T @ u
    v = v / max(np.linalg.norm(v), EPS)
    u = M @ v
    return u / max(np.linalg.norm(u), EPS), v


def spectral_sigma(W, u, v):
    return float(u @ (W.reshape(W.shape[0], -1) @ v))


def spectral_fold(W, u, v, training=False, mutant=None):
    """-> (W / sigma, u, v): in training mode after one iteration; the mutant takes sigma before it"""
    before = spectral_sigma(W, u, v)
    if training:
        u, v = spectral_iterate(W, u, v)
    return W / (before if mutant == "sigma_before_iteration" else spectral_sigma(W, u, v)), u, v


def spectral_gradient(W, u, v, dw):
    """the gradient of weight_orig from the folded weight's, u and v held constant: dw / sigma - <dw, W> / sigma^2 u v^T"""
    sigma = spectral_sigma(W, u, v)
    return dw / sigma - ((dw * W).sum() / sigma ** 2) * np.outer(u, v).reshape(W.shape)


def spectral_w_ulps(W, u, v):
    """how many u a float32 W / sigma may be off, relative to |W|: the matrix-vector product and the dot of sigma in their worst case, and the division"""
    M = np.abs(W.reshape(W.shape[0], -1))
    return int(np.ceil((sum(M.shape) + 2) * (np.abs(u) @ (M @ np.abs(v))) / abs(spectral_sigma(W, u, v)))) + 3


# ---- the multi-scale discriminator with its three losses, and the combined one -----------------------------------------------------------------------------------

def msd_reference(cfg, wss, real, fake, count=None, w_adv=1.0, w_fm=2.0, w_ulps=None):
    """wss: the weights per scale (folded).  count: the number of discriminators the losses are averaged over (default: the scales).  w_ulps [scale]: the
    ulps the device's folded weights may be off.  -> as hfgd_ref.mpd_reference: adv, fm, d_real, d_fake with their bounds, gx / gx_e per fake utterance,
    unsure: the worst share of unsure cells of any array (mask and L1 cells together)"""
    S = len(wss)
    N = S if count is None else count
    out = dict(adv=0.0, adv_e=0.0, fm=0.0, fm_e=0.0, d_real=0.0, d_real_e=0.0, d_fake=0.0, d_fake_e=0.0, unsure=0.0, mask_unsure=0.0, shares=[])
    chain_r, chain_f = [pool_chain(x, S - 1) for x in real], [pool_chain(x, S - 1) for x in fake]
    gx, gx_e = [np.zeros(len(x)) for x in fake], [np.zeros(len(x)) for x in fake]
    for i, ws in enumerate(wss):
        wu = 0 if w_ulps is None else w_ulps[i]
        fr = forward(cfg, ws, [c[i][0] for c in chain_r], w_ulps=wu, e_in=[c[i][1] for c in chain_r])
        ff = forward(cfg, ws, [c[i][0] for c in chain_f], w_ulps=wu, e_in=[c[i][1] for c in chain_f])
        L = len(ws) - 1
        sc_r, sc_f = [r["h"][-1] for r in fr], [r["h"][-1] for r in ff]
        e_r, e_f = [r["e"][-1] for r in fr], [r["e"][-1] for r in ff]
        out["adv"] += D.mse(sc_f, 1.0) / N
        out["adv_e"] += D.mse_bound(sc_f, e_f, 1.0) / N
        out["d_real"] += D.mse(sc_r, 1.0) / N
        out["d_real_e"] += D.mse_bound(sc_r, e_r, 1.0) / N
        out["d_fake"] += D.mse(sc_f, 0.0) / N
        out["d_fake_e"] += D.mse_bound(sc_f, e_f, 0.0) / N
        n_sc = sum(s.size for s in sc_f)
        ds = [w_adv * 2.0 * (s - 1.0) / (n_sc * N) for s in sc_f]
        eg = [w_adv * 2.0 * e / (n_sc * N) + 8 * U * np.abs(d) for e, d in zip(e_f, ds)]
        extras, e_extras = [[] for _ in fake], [[] for _ in fake]
        mask_unsure = unsure_cells(ff)
        for l in range(L):
            cells = sum(r["h"][l].size for r in ff)
            c = w_fm / (cells * L * N)
            kinks, masks = 0, 0
            for u in range(len(fake)):
                d, tol = ff[u]["h"][l] - fr[u]["h"][l], ff[u]["e"][l] + fr[u]["e"][l]
                near = np.abs(d) <= tol
                kinks += int((near | mask_unsure[l][u]).sum())
                masks += int(mask_unsure[l][u].sum())
                extras[u].append(c * np.sign(d))
                e_extras[u].append(np.where(near, 2 * c, 8 * U * c))
                out["fm"] += np.abs(d).sum() / (cells * L * N)
                out["fm_e"] += tol.sum() / (cells * L * N) + 8 * U * np.abs(d).sum() / (cells * L * N)
            out["unsure"], out["mask_unsure"] = max(out["unsure"], kinks / cells), max(out["mask_unsure"], masks / cells)
            out["shares"].append((i, l, kinks / cells, masks / cells))
        bw = backward(cfg, ws, ff, ds, extras=extras, end_to_end=True, eg_in=eg, e_extras=e_extras, w_ulps=wu)
        for u in range(len(fake)):
            g, e = bw["gx"][u], bw["gx_e"][u]
            for j in range(i, 0, -1):  # down through the poolings' adjoints to the waveform
                T = len(chain_f[u][j - 1][0])
                g, e = pool_adjoint(g, T), 3 * U * pool_adjoint(np.abs(g), T) + pool_adjoint(e, T)
            gx[u] += g
            gx_e[u] += e + 2 * U * np.abs(gx[u])
    out["gx"], out["gx_e"] = gx, gx_e
    return out


def combined_reference(cfg_s, wss_s, cfg_p, wss_p, real, fake, periods, w_adv=1.0, w_fm=2.0, w_ulps=None):
    """the scales followed by the periods, every loss averaged over all of them"""
    S, P = len(wss_s), len(periods)
    N = S + P
    out = msd_reference(cfg_s, wss_s, real, fake, count=N, w_adv=w_adv, w_fm=w_fm, w_ulps=w_ulps)
    per = D.mpd_reference(cfg_p, wss_p, real, fake, periods, w_adv=w_adv * P / N, w_fm=w_fm * P / N)
    for key in ("adv", "fm", "d_real", "d_fake"):
        out[key] += per[key] * P / N
        out[key + "_e"] += per[key + "_e"] * P / N
    out["unsure"] = max(out["unsure"], per["unsure"])
    for u in range(len(fake)):
        out["gx"][u] = out["gx"][u] + per["gx"][u]
        out["gx_e"][u] = out["gx_e"][u] + per["gx_e"][u] + 2 * U * np.abs(out["gx"][u])
    return out


# ---- the second statement: torch.nn.functional.conv1d(groups=), F.avg_pool1d and autograd, float64 on the CPU --------------------------------------------------

def torch_statement(cfg, ws, xs, dscores=None, extras=None, pooled=0):
    """-> dict(h [utt][l] as forward()'s h on the waveform pooled `pooled` times; with dscores also gx [utt] (to the unpooled waveform), dw, db per layer).
    The loss is sum dscore scores + sum_l sum extra_l map_l."""
    import torch
    import torch.nn.functional as F

    geo = geometry(cfg)
    T64 = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)
    Wt = [T64(W) for W, _ in ws]
    bt = [None if b is None else T64(b) for _, b in ws]
    to_seg = lambda a: a.permute(0, 2, 1)  # [1, C, T] -> [1, T, C]
    out, total, xts = dict(h=[], gx=[], x=[]), 0.0, []
    for u, x in enumerate(xs):
        xt = T64(x)
        xts.append(xt)
        h = xt[None, None, :]
        for _ in range(pooled):
            h = F.avg_pool1d(h, 4, 2, 2)
        out["x"].append(h[0, 0].detach().numpy())
        hs = []
        for l, (ci, co, k, s, pad, gr) in enumerate(geo):
            h = F.conv1d(h, Wt[l], bt[l], stride=s, padding=pad, groups=gr)
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
        out["dw"] = [w.grad.numpy() for w in Wt]
    return out


# ---- the cases the CPU and the GPU tests share ---------------------------------------------------------------------------------------------------------------------

def chain_case(name, gain=GAIN):
    """one scale discriminator end to end on a chain configuration: the inputs, the float64 forward, given gradients for every output, and the float64
    backward with its running bounds"""
    cfg = CHAINS[name]
    seed = 11 * (1 + "AB".index(name))
    ws, xs = weights(cfg, seed, gain), signals(LENS, 40 + seed)
    fw = forward(cfg, ws, xs)
    ds, ex = given_gradients(fw, seed)
    bw = backward(cfg, ws, fw, ds, extras=ex, end_to_end=True)
    return dict(cfg=cfg, ws=ws, xs=xs, fw=fw, ds=ds, ex=ex, bw=bw)


def spectral_state(W, seed, iterations=30):
    """(u, v) for W after `iterations` power iterations from a random start: where a trained module's buffers stand"""
    rng = np.random.default_rng(7000 + seed)
    u, v = rng.standard_normal(W.shape[0]), rng.standard_normal(W[0].size)
    u, v = u / np.linalg.norm(u), v / np.linalg.norm(v)
    for _ in range(iterations):
        u, v = spectral_iterate(W, u, v)
    return f32(u), f32(v)


def msd_inputs(gain=GAIN, scales=3):
    """the multi-scale case on MSD_CFG: discriminator 0 under spectral norm (eval mode: its stored u, v), the others plain.  orig [scale]: the stored
    weights; uv: discriminator 0's buffers per layer; fold64: discriminator 0's folded weights in float64"""
    orig = [weights(MSD_CFG, 60 + i, gain) for i in range(scales)]
    uv = [spectral_state(W, 3 * l) for l, (W, _) in enumerate(orig[0])]
    fold64 = [spectral_fold(W, u, v)[0] for (W, _), (u, v) in zip(orig[0], uv)]
    return dict(cfg=MSD_CFG, orig=orig, uv=uv, fold64=fold64, real=signals(MSD_LENS, 17), fake=signals(MSD_LENS, 18))


def msd_case(folded=None):
    """msd_inputs() and the reference on them.  A worst-case bound of a float32 sigma (spectral_w_ulps: thousands of u) would swamp every forward bound, so the
    reference runs on the float32 folded weights themselves: folded [scale][layer] = the device's own (the GPU test checks them against the float64 fold
    within that bound first), or by default the float64 fold rounded to float32 for discriminator 0 and the stored weights for the others."""
    m = msd_inputs()
    if folded is None:
        folded = [[f32(W) for W in m["fold64"]]] + [[W for W, _ in ws] for ws in m["orig"][1:]]
    m["wss"] = [[(W, b) for W, (_, b) in zip(fs, ws)] for fs, ws in zip(folded, m["orig"])]
    m["ref"] = msd_reference(m["cfg"], m["wss"], m["real"], m["fake"])
    return m
