"""The Parallel WaveGAN discriminator (include/fcl_hip.h "Parallel WaveGAN discriminator") stated in float64 numpy: the forward pass, the
backward pass on given stored activations, and running error bounds for an exact-fp32 evaluation of either, computed from the reference alone.  No package
code.  A second statement at the end uses torch.nn.functional.conv1d and autograd in float64 on the CPU.

The network: layer i = 0 .. L - 2 is Conv1d(cin_i -> C, k, dilation d_i, padding (k - 1) / 2 d_i) + LeakyReLU(slope); cin_0 = 1, d_0 = 1, d_i = i for
dilation_factor 1, else dilation_factor ** i; layer L - 1 is Conv1d(C -> 1, k, dilation 1) without activation.  Weights are torch's [cout, cin, k].

Bounds (u = 2^-24; worst case, so nothing is added to them):
  forward, per cell:   e_l = (k cin_l + 2 + w_ulps) u (sum |w| |h_{l-1}| + |b|) + sum |w| e_{l-1},  e_{-1} = 0 (the waveform is given in float32).
                       k cin roundings of the contraction in any order, one of the bias, one of the slope; LeakyReLU is 1-Lipschitz, so the bound of the
                       pre-activation also holds after it.  w_ulps: the weights themselves are only known to w_ulps u |w| (end to end under weight norm,
                       where the device folds v g / ||v|| in float32: k cin / 2 + 1 for the norm, a division and a product -> k cin + 4 covers it).
  input gradient:      the same recursion downwards on the gradient of the pre-activations: eg_{l-1} = m ((k cout_l + 2 + w_ulps) u sum |w| |g_l| + sum |w| eg_l),
                       m the LeakyReLU derivative read from the GIVEN activation (1 where h > 0, else the slope; h == 0 takes the slope) -- on given
                       activations the mask is a function of the inputs and no kink ambiguity arises.
  weight gradients:    (n_samples + 2) u sum_t |g| |h| + sum_t eg |h| (+ sum_t (|g| + eg) eh where the activations themselves carry an error eh: end to
                       end); the bias gradient likewise with h = 1.  n_samples counts the whole batch; valid for any summation order."""
import numpy as np

U = 2.0 ** -24
LENS = (1, 5, 130, 257, 77)  # shorter than the largest dilation, boundaries inside a tile, a total (470) that is no multiple of a tile
CONFIGS = {
    "default": dict(conv_channels=64, kernel_size=3, layers=10, dilation_factor=1, bias=True, negative_slope=0.2),
    "c16k5f2": dict(conv_channels=16, kernel_size=5, layers=5, dilation_factor=2, bias=True, negative_slope=0.2),
    "c128relu": dict(conv_channels=128, kernel_size=3, layers=3, dilation_factor=1, bias=False, negative_slope=0.0),
    "c96k5": dict(conv_channels=96, kernel_size=5, layers=3, dilation_factor=1, bias=True, negative_slope=0.2),  # the half-width split with 3 tiles, pwd_dw_kernel<6>
    "c112": dict(conv_channels=112, kernel_size=3, layers=3, dilation_factor=1, bias=True, negative_slope=0.2),  # the 7-tile arm
}
CASES = [(name, LENS) for name in CONFIGS]
MUTANTS = ("taps_not_reversed", "dilation_plus_one", "across_boundary", "slope_one_at_zero", "no_bias_gradient", "d_i_is_i_plus_1")

# end to end (device forward then device backward against float64 forward then float64 backward) no mask may flip: the cases are those where the
# reference alone finds no pre-activation within its own forward bound of zero, in 100 % of the cells.  Found by first_clean_seed() among the first 80.
# C 16, 5 layers, factor 2, 90 samples.  With kernel size 5 (the kernel case above) no seed among the first 80 is clean -- the bound of the fourth
# layer's cells reaches 1e-2 -- so the end-to-end cases use kernel size 3: seeds 52, 76, 78 are clean for the generator's loss, 52 for the discriminator's
# (two batches, twice the cells).
E2E_CFG = dict(conv_channels=16, kernel_size=3, layers=5, dilation_factor=2, bias=True, negative_slope=0.2)
E2E_LENS = (37, 53)
SEEDS = {"generator": 52, "discriminator": 52}  # seed of e2e_inputs per loss


def geometry(cfg, mutant=None):
    """[(cin, cout, dilation)] per layer"""
    C, L, f = cfg["conv_channels"], cfg["layers"], cfg["dilation_factor"]
    geo = []
    for i in range(L - 1):
        j = i + 1 if mutant == "d_i_is_i_plus_1" and i >= 1 else i
        d = 1 if i == 0 else (j if f == 1 else f ** j)
        if mutant == "dilation_plus_one" and i >= 1:
            d += 1
        geo.append((1 if i == 0 else C, C, d))
    return geo + [(C, 1, 1)]


def weights(cfg, seed):
    """per layer (W [cout, cin, k], b [cout] or None): float32 values held in float64; Kaiming-scaled weights, biases that are not zero"""
    rng = np.random.default_rng(1000 + seed)
    out = []
    for ci, co, _ in geometry(cfg):
        W = (rng.standard_normal((co, ci, cfg["kernel_size"])) * np.sqrt(2.0 / (ci * cfg["kernel_size"]))).astype(np.float32).astype(np.float64)
        b = (0.1 * rng.standard_normal(co)).astype(np.float32).astype(np.float64) if cfg["bias"] else None
        out.append((W, b))
    return out


def signals(lens, seed):
    """one float32 waveform per utterance (held in float64): a sine plus noise within [-1, 1]"""
    rng = np.random.default_rng(2000 + seed)
    out = []
    for i, n in enumerate(lens):
        t = np.arange(n)
        x = 0.5 * np.sin(2 * np.pi * (0.01 + 0.013 * i) * t + i) + 0.3 * rng.standard_normal(n)
        out.append(np.clip(x, -1, 1).astype(np.float32).astype(np.float64))
    return out


def given_gradient(lens, seed):
    """a float32 dscore per utterance"""
    rng = np.random.default_rng(3000 + seed)
    return [rng.standard_normal(n).astype(np.float32).astype(np.float64) for n in lens]


def _taps(k, d, T):
    """(j, shift, t0, t1): output rows [t0, t1) read rows [t0 + shift, t1 + shift) under tap j; everything else of the tap falls outside the utterance"""
    for j in range(k):
        s = (j - (k - 1) // 2) * d
        t0, t1 = max(0, -s), min(T, T - s)
        if t1 > t0:
            yield j, s, t0, t1


def conv(h, W, b, d):
    """h [T, cin] -> [T, cout] = b + sum_j h[t + (j - (k - 1) / 2) d] W[:, :, j]^T, zero outside [0, T)"""
    T = h.shape[0]
    out = np.zeros((T, W.shape[0])) + (0.0 if b is None else b)
    for j, s, t0, t1 in _taps(W.shape[2], d, T):
        out[t0:t1] += h[t0 + s : t1 + s] @ W[:, :, j].T
    return out


def conv_dx(g, W, d, mutant=None):
    """g [T, cout] -> [T, cin]: d loss / d input = sum_j g[r - shift_j] W[:, :, j] (the taps reversed); the mutant forgets the reversal"""
    T = g.shape[0]
    out = np.zeros((T, W.shape[1]))
    for j, s, t0, t1 in _taps(W.shape[2], d, T):
        if mutant == "taps_not_reversed":
            out[t0:t1] += g[t0 + s : t1 + s] @ W[:, :, j]
        else:
            out[t0 + s : t1 + s] += g[t0:t1] @ W[:, :, j]
    return out


def conv_dw(g, h, k, d):
    """-> [cout, cin, k]: sum_t g[t, co] h[t + shift_j, ci]"""
    out = np.zeros((g.shape[1], h.shape[1], k))
    for j, s, t0, t1 in _taps(k, d, g.shape[0]):
        out[:, :, j] = g[t0:t1].T @ h[t0 + s : t1 + s]
    return out


def leaky(v, slope):
    return np.where(v > 0, v, slope * v)


def forward(cfg, ws, xs, mutant=None, w_ulps=0):
    """per utterance dict(pre, h, e): pre[l] the pre-activations, h[l] the post-activations (h[L - 1] = the scores [T, 1]), e[l] the bound of a cell of
    either; mutants: "across_boundary" runs the packed batch as one utterance, the dilation mutants change the geometry"""
    geo, slope = geometry(cfg, mutant), cfg["negative_slope"]
    if mutant == "across_boundary":
        joined = forward(cfg, ws, [np.concatenate(xs)], None, w_ulps)[0]
        cuts = np.cumsum([len(x) for x in xs])[:-1]
        parts = {key: [np.split(v, cuts) for v in joined[key]] for key in joined}
        return [{key: [layer[i] for layer in parts[key]] for key in parts} for i in range(len(xs))]
    out = []
    for x in xs:
        h, e = x[:, None], np.zeros((len(x), 1))
        r = dict(pre=[], h=[], e=[])
        for l, ((W, b), (ci, co, d)) in enumerate(zip(ws, geo)):
            pre = conv(h, W, b, d)
            e = (W.shape[2] * ci + 2 + w_ulps) * U * conv(np.abs(h), np.abs(W), None if b is None else np.abs(b), d) + conv(e, np.abs(W), None, d)
            h = leaky(pre, slope) if l < len(geo) - 1 else pre
            r["pre"].append(pre), r["h"].append(h), r["e"].append(e)
        out.append(r)
    return out


def layer_forward(cfg, ws, l, hin):
    """one layer on a GIVEN float32 input hin [T, cin] of one utterance -> (h [T, cout], its bound): the first term of the recursion alone, so a deep
    layer is held as tightly as the first"""
    (W, b), (ci, co, d) = ws[l], geometry(cfg)[l]
    pre = conv(hin, W, b, d)
    e = (W.shape[2] * ci + 2) * U * conv(np.abs(hin), np.abs(W), None if b is None else np.abs(b), d)
    return (leaky(pre, cfg["negative_slope"]) if l < cfg["layers"] - 1 else pre), e


def kink_free_share(fw):
    """the share of the activated cells whose pre-activation lies further from zero than its own bound (1.0: no mask can flip)"""
    ok = tot = 0
    for r in fw:
        for pre, e in zip(r["pre"][:-1], r["e"][:-1]):
            ok, tot = ok + int((np.abs(pre) > e).sum()), tot + pre.size
    return ok / tot


def backward(cfg, ws, xs, hs, dscores, mutant=None, eg_in=None, ehs=None, w_ulps=0):
    """xs [utt][T]; hs [utt][l] the GIVEN stored activations h_0 .. h_{L-2} [T, C]; dscores [utt][T] -> dict(gx, gx_e per utterance; dw, dw_e, db, db_e per
    layer, summed over the batch).  eg_in [utt][T]: the error the given dscore already carries; ehs [utt][l]: the error of the stored activations (both
    end to end only)."""
    geo, slope, k = geometry(cfg, mutant), cfg["negative_slope"], cfg["kernel_size"]
    n = sum(len(x) for x in xs)
    L = len(geo)
    z = lambda: [np.zeros(W.shape) for W, _ in ws]
    zb = lambda: [np.zeros(W.shape[0]) for W, _ in ws]
    r = dict(gx=[], gx_e=[], dw=z(), dw_e=z(), db=zb(), db_e=zb())
    for u, x in enumerate(xs):
        g = dscores[u][:, None]
        eg = np.zeros_like(g) if eg_in is None else eg_in[u][:, None]
        for l in range(L - 1, -1, -1):
            (W, _), (ci, co, d) = ws[l], geo[l]
            below = x[:, None] if l == 0 else hs[u][l - 1]
            r["dw"][l] += conv_dw(g, below, k, d)
            r["dw_e"][l] += (n + 2) * U * conv_dw(np.abs(g), np.abs(below), k, d) + conv_dw(eg, np.abs(below), k, d)
            if ehs is not None and l > 0:
                r["dw_e"][l] += conv_dw(np.abs(g) + eg, ehs[u][l - 1], k, d)
            if mutant != "no_bias_gradient":
                r["db"][l] += g.sum(0)
            r["db_e"][l] += (n + 2) * U * np.abs(g).sum(0) + eg.sum(0)
            gin = conv_dx(g, W, d, mutant)
            ein = (k * co + 2 + w_ulps) * U * conv_dx(np.abs(g), np.abs(W), d) + conv_dx(eg, np.abs(W), d)
            if l > 0:
                m = np.where(below >= 0 if mutant == "slope_one_at_zero" else below > 0, 1.0, slope)
                g, eg = m * gin, m * ein
            else:
                r["gx"].append(gin[:, 0]), r["gx_e"].append(ein[:, 0])
    return r


# ---- the end-to-end cases: the adversarial losses on the scores, under weight norm ------------------------------------------------------------------

def e2e_inputs(seed, loss):
    """-> (cfg, vs, gs, bs, real, fake): weight-norm parameters (float32 values) and one or two batches of E2E_LENS"""
    cfg = E2E_CFG
    rng = np.random.default_rng(4000 + seed)
    ws = weights(cfg, 50 + seed)
    vs = [W for W, _ in ws]
    gs = [(np.sqrt((W ** 2).sum((1, 2))) * (0.8 + 0.4 * rng.random(W.shape[0]))).astype(np.float32).astype(np.float64) for W in vs]
    bs = [b for _, b in ws]
    fake = signals(E2E_LENS, 70 + seed)
    real = signals(E2E_LENS, 170 + seed) if loss == "discriminator" else None
    return cfg, vs, gs, bs, real, fake


def fold(v, g):
    """w = v g / ||v|| over dims 1, 2"""
    return v * (g / np.sqrt((v ** 2).sum((1, 2))))[:, None, None]


def fold_ulps(cfg, layer):
    ci = geometry(cfg)[layer][0]
    return cfg["kernel_size"] * ci + 4


def e2e_reference(seed, loss):
    """generator: mean (p_fake - 1)^2 -> the waveform gradient per utterance; discriminator: mean (p_real - 1)^2 + mean p_fake^2 -> the gradients of
    weight_g, weight_v and the biases.  Each with its bound: the forward bound of the scores enters the given gradient, the activations' bounds enter the
    weight gradients, and the weight-norm chain (evaluated by the device in float32 torch operations) adds its Jacobian applied to the bound of dW plus
    (2 k cin + 16) u of its own terms."""
    cfg, vs, gs, bs, real, fake = e2e_inputs(seed, loss)
    ws = [(fold(v, g), b) for v, g, b in zip(vs, gs, bs)]
    w_ulps = max(fold_ulps(cfg, l) for l in range(len(ws)))
    xs = fake if real is None else real + fake
    fw = forward(cfg, ws, xs, w_ulps=w_ulps)
    L = len(ws)
    scores, es = [r["h"][-1][:, 0] for r in fw], [r["e"][-1][:, 0] for r in fw]
    nf = sum(len(x) for x in fake)
    if real is None:
        ds = [2.0 * (p - 1.0) / nf for p in scores]
        value = sum(((p - 1.0) ** 2).sum() for p in scores) / nf
        eg = [2.0 * e / nf + 4 * U * np.abs(d) for e, d in zip(es, ds)]
    else:
        R, nr = len(real), sum(len(x) for x in real)
        ds = [2.0 * (p - 1.0) / nr for p in scores[:R]] + [2.0 * p / nf for p in scores[R:]]
        value = sum(((p - 1.0) ** 2).sum() for p in scores[:R]) / nr + sum((p ** 2).sum() for p in scores[R:]) / nf
        eg = [2.0 * e / (nr if i < R else nf) + 4 * U * np.abs(d) for i, (e, d) in enumerate(zip(es, ds))]
    hs, ehs = [r["h"][: L - 1] for r in fw], [r["e"][: L - 1] for r in fw]
    bw = backward(cfg, ws, xs, hs, ds, eg_in=eg, ehs=ehs, w_ulps=w_ulps)
    out = dict(share=kink_free_share(fw), value=value, gx=bw["gx"], gx_e=bw["gx_e"], db=bw["db"], db_e=bw["db_e"], dg=[], dg_e=[], dv=[], dv_e=[], xs=xs,
               vs=vs, gs=gs, bs=bs, real=real, fake=fake, cfg=cfg)
    for l, (v, g) in enumerate(zip(vs, gs)):
        dw, ew = bw["dw"][l], bw["dw_e"][l]
        nrm = np.sqrt((v ** 2).sum((1, 2)))
        c = (2 * fold_ulps(cfg, l) + 8) * U
        dot = lambda a, b: (a * b).sum((1, 2))
        col = lambda a: a[:, None, None]
        out["dg"].append(dot(dw, v) / nrm)
        out["dg_e"].append(dot(ew, np.abs(v)) / nrm + c * dot(np.abs(dw), np.abs(v)) / nrm)
        out["dv"].append(col(g / nrm) * dw - col(g * dot(dw, v) / nrm ** 3) * v)
        mag = lambda a: col(g / nrm) * a + col(g * dot(a, np.abs(v)) / nrm ** 3) * np.abs(v)
        out["dv_e"].append(mag(ew) + c * mag(np.abs(dw)))
    return out


def first_clean_seed(loss, tries=80):
    for seed in range(tries):
        if e2e_reference(seed, loss)["share"] == 1.0:
            return seed
    return None


# ---- the second statement: torch.nn.functional.conv1d and autograd in float64 on the CPU -------------------------------------------------------------

def torch_statement(cfg, ws, xs, dscores=None):
    """-> dict(h [utt][l] as forward()'s h ([T, C], the scores [T, 1]); with dscores also gx [utt], dw, db per layer)"""
    import torch
    import torch.nn.functional as F

    geo, k = geometry(cfg), cfg["kernel_size"]
    Wt = [torch.tensor(W, dtype=torch.float64, requires_grad=True) for W, _ in ws]
    bt = [None if b is None else torch.tensor(b, dtype=torch.float64, requires_grad=True) for _, b in ws]
    out = dict(h=[], gx=[])
    for u, x in enumerate(xs):
        xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
        h, hs = xt[None, None, :], []
        for l, (ci, co, d) in enumerate(geo):
            h = F.conv1d(h, Wt[l], bt[l], dilation=d, padding=(k - 1) // 2 * d)
            if l < len(geo) - 1:
                h = F.leaky_relu(h, cfg["negative_slope"])
            hs.append(h)
        out["h"].append([a.detach()[0].T.numpy() for a in hs])
        if dscores is not None:
            h[0, 0].backward(torch.tensor(dscores[u], dtype=torch.float64))
            out["gx"].append(xt.grad.numpy())
    if dscores is not None:
        out["dw"] = [w.grad.numpy() for w in Wt]
        out["db"] = [None if b is None else b.grad.numpy() for b in bt]
    return out


def torch_weight_norm_statement(v, g):
    """torch.nn.utils.weight_norm on a Conv1d holding (g, v) -> its folded weight, float64"""
    import torch

    conv = torch.nn.Conv1d(v.shape[1], v.shape[0], v.shape[2]).double()
    conv = torch.nn.utils.weight_norm(conv)
    with torch.no_grad():
        conv.weight_v.copy_(torch.tensor(v))
        conv.weight_g.copy_(torch.tensor(g).reshape(-1, 1, 1))
    conv(torch.zeros(1, v.shape[1], v.shape[2], dtype=torch.float64))  # the hook recomputes .weight
    return conv.weight.detach().numpy()
