"""Float64 numpy statement of the Parallel WaveGAN generator's residual block and stack, forward and backward, with derived worst-case bounds (DESIGN.md
6m; the contract of include/fcl_hip.h "Parallel WaveGAN generator, training form").  Arrays are packed [samples, C] with the utterance lengths `lens`;
a block's weights are a dict conv [2R, R, k], b_conv [2R], aux [2R, A], out [R, R], b_out [R], skip [R, R], b_skip [R] in torch's orientation
(output channel first).

Bounds, u = 2^-24.  A contraction of K terms evaluated in float32 in any order is within (K + c) u sum |w| |x| of its exact value, c counting the extra
roundings of its epilogue; an input error e propagates as |w| e.  The gate: |da| <= e_z + E_T (|tanh'| <= 1), |db| <= e_z / 4 + E_S (|sigmoid'| <= 1/4),
E_T / E_S the device functions' own errors, measured on the MI355X and set to twice the worst value seen, rounded up to a power of two
times u.  Every function takes the input errors (None: exact inputs) -- with None it gives the first term, the bound of one launch on given inputs.
The gate's derivative has no kink: no cell is excluded anywhere."""
import math

import numpy as np

U = 2.0 ** -24
E_T = 4 * U  # tanhf: worst seen 1.34 u over the 24 block-level cells of test_gpu_pwg_generator.py
E_S = 4 * U  # 1 / (1 + expf(-z)): worst seen 1.49 u
SQH = math.sqrt(0.5)

LENS = (1, 5, 130, 1100, 77)  # an utterance shorter than every dilation above 1; edges inside a 128-row tile; 1313 rows: no multiple of a tile; one
#                               utterance that crosses a 1024-sample weight-gradient chunk and exceeds dilation 512
DILATIONS = (1, 2, 64, 512)
BLOCK_CONFIGS = {"r64_a80_k3": (64, 80, 3), "r16_a16_k5": (16, 16, 5), "r32_a128_k3": (32, 128, 3)}
SMALL_STACK = dict(layers=4, stacks=2, residual_channels=16, gate_channels=32, skip_channels=16, aux_channels=16, kernel_size=3, upsample_scales=(2,))
MUTANTS_FWD = ("dilation_halved", "across_edge", "aux_dropped")
MUTANTS_BWD = ("taps_not_reversed", "dc_overwritten", "no_1_minus_a2", "no_sqrt_half_residual", "missing_bias_gradient")


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


def block_weights(sd, l, dt=np.float64):
    p = "conv_layers.%d." % l
    f = lambda k: np.asarray(sd[p + k], dtype=dt)
    return dict(conv=f("conv.weight"), b_conv=f("conv.bias"), aux=f("conv1x1_aux.weight")[:, :, 0], out=f("conv1x1_out.weight")[:, :, 0],
                b_out=f("conv1x1_out.bias"), skip=f("conv1x1_skip.weight")[:, :, 0], b_skip=f("conv1x1_skip.bias"))


def dilations(cfg):
    per = cfg["layers"] // cfg["stacks"]
    return [2 ** (l % per) for l in range(cfg["layers"])]


def _zero(e, like):
    return np.zeros(like.shape) if e is None else e


def gate_forward(w, x, c, lens, d, ex=None, mutant=None, dt=np.float64):
    """-> z, a = tanh(z[:, :R]), b = sigmoid(z[:, R:]) and their bounds e_z, e_a, e_b"""
    f = lambda v: np.asarray(v, dtype=dt)
    R, k, A = x.shape[1], w["conv"].shape[2], c.shape[1]
    dd = max(d // 2, 1) if mutant == "dilation_halved" else d
    z = np.tile(f(w["b_conv"]), (len(x), 1))
    az, ein = np.tile(np.abs(w["b_conv"]).astype(np.float64), (len(x), 1)), np.zeros((len(x), 2 * R))
    for j in range(k):
        sh, Wj = (j - (k - 1) // 2) * dd, w["conv"][:, :, j].T
        xs = shift(f(x), lens, sh, mutant == "across_edge")
        z = z + xs @ f(Wj)
        az += np.abs(xs).astype(np.float64) @ np.abs(Wj)
        if ex is not None:
            ein += shift(ex, lens, sh) @ np.abs(Wj)
    if mutant != "aux_dropped":
        z = z + f(c) @ f(w["aux"].T)
    az += np.abs(c).astype(np.float64) @ np.abs(w["aux"].T)
    e_z = (k * R + A + 2) * U * az + ein
    a, b = np.tanh(z[:, :R]), 1.0 / (1.0 + np.exp(-z[:, R:]))
    return dict(z=z, a=a, b=b, e_z=e_z, e_a=e_z[:, :R] + E_T, e_b=e_z[:, R:] / 4 + E_S)


def _gate_product_error(a, b, ea, eb):
    return np.abs(b) * ea + np.abs(a) * eb + ea * eb


def out_forward(w, x, a, b, skips_in, ex=None, ea=None, eb=None, es=None, dt=np.float64):
    """x_out = (g out^T + b_out + x) sqrt(.5), skips = (skips_in +) g skip^T + b_skip (skips_in None: the first block) and their bounds"""
    f = lambda v: np.asarray(v, dtype=dt)
    R = x.shape[1]
    g = f(a) * f(b)
    eg = _gate_product_error(a, b, _zero(ea, a), _zero(eb, b))
    ag = np.abs(g).astype(np.float64)
    x_out = (g @ f(w["out"].T) + f(w["b_out"]) + f(x)) * dt(SQH)
    e_x = SQH * ((R + 6) * U * (ag @ np.abs(w["out"].T) + np.abs(w["b_out"]) + np.abs(x)) + eg @ np.abs(w["out"].T) + _zero(ex, x))
    s = g @ f(w["skip"].T) + f(w["b_skip"])
    e_s = (R + 4) * U * (ag @ np.abs(w["skip"].T) + np.abs(w["b_skip"])) + eg @ np.abs(w["skip"].T)
    if skips_in is not None:
        s = f(skips_in) + s
        e_s = e_s + _zero(es, s) + U * np.abs(s)
    return dict(x_out=x_out, skips=s, e_x=e_x, e_s=e_s)


def block_backward(w, x, c, a, b, dxo, ds, lens, d, err=None, mutant=None, dt=np.float64):
    """on the stored a, b and the given dxo (None: the last block) and ds -> dz, dx, dc (this block's term), the seven parameter gradients (torch's
    orientation) and the bound of each (e_*).  err: dict of the inputs' errors ex, ea, eb, edxo (None: exact inputs, the first term)."""
    f = lambda v: np.asarray(v, dtype=dt)
    err = err or {}
    n, R, k = len(x), x.shape[1], w["conv"].shape[2]
    ex, ea, eb = _zero(err.get("ex"), x), _zero(err.get("ea"), a), _zero(err.get("eb"), b)
    a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
    a_, b_, ds_ = f(a), f(b), f(ds)
    dg, adg, edg_in = ds_ @ f(w["skip"]), np.abs(ds) @ np.abs(w["skip"]), np.zeros((n, R))
    if dxo is not None:
        sx = f(dxo) * dt(SQH)
        dg = sx @ f(w["out"]) + dg
        adg = adg + SQH * np.abs(dxo) @ np.abs(w["out"])
        edxo = _zero(err.get("edxo"), dxo)
        edg_in = SQH * edxo @ np.abs(w["out"])
    e_dg = (2 * R + 3) * U * adg + edg_in
    one = dt(1.0)
    fa = b_ if mutant == "no_1_minus_a2" else b_ * (one - a_ * a_)
    fb = a_ * b_ * (one - b_)
    fa64, fb64 = b64 * (1 - a64 * a64), a64 * b64 * (1 - b64)
    e_fa = 2 * U * np.abs(b64) + 2 * U * np.abs(fa64) + eb * np.abs(1 - a64 * a64) + (np.abs(b64) + eb) * (2 * np.abs(a64) * ea + ea * ea)
    ep = _gate_product_error(a64, b64, ea, eb)
    e_fb = U * np.abs(a64 * b64) + 3 * U * np.abs(fb64) + ep * np.abs(1 - b64) + np.abs(a64 * b64) * eb + ep * eb
    dz = np.concatenate([dg * fa, dg * fb], axis=1)
    fac, e_fac = np.concatenate([fa64, fb64], axis=1), np.concatenate([e_fa, e_fb], axis=1)
    dg2, e_dg2 = np.abs(np.concatenate([dg, dg], axis=1)).astype(np.float64), np.concatenate([e_dg, e_dg], axis=1)
    e_dz = e_dg2 * np.abs(fac) + dg2 * e_fac + e_dg2 * e_fac + U * np.abs(dz)
    return dict(dz=dz, e_dz=e_dz, **from_dz(w, x, c, a, b, dxo, ds, dz, lens, d, dict(err, edz=e_dz), mutant, dt))


def from_dz(w, x, c, a, b, dxo, ds, dz, lens, d, err=None, mutant=None, dt=np.float64):
    """what the launches after pwt_dz_kernel compute from dz (and x, c, a, b, dxo, ds): dx, dc, the parameter gradients, and their bounds"""
    f = lambda v: np.asarray(v, dtype=dt)
    err = err or {}
    n, R, k = len(x), x.shape[1], w["conv"].shape[2]
    ex, ea, eb, e_dz = _zero(err.get("ex"), x), _zero(err.get("ea"), a), _zero(err.get("eb"), b), _zero(err.get("edz"), dz)
    edxo = None if dxo is None else _zero(err.get("edxo"), dxo)
    dz_, adz = f(dz), np.abs(dz).astype(np.float64)
    dx, adx, edx = np.zeros((n, R), dt), np.zeros((n, R)), np.zeros((n, R))
    dconv, e_dconv = np.zeros(w["conv"].shape, dt), np.zeros(w["conv"].shape)
    for j in range(k):
        sh, Wj = (j - (k - 1) // 2) * d, w["conv"][:, :, j]  # [2R, R]
        back = sh if mutant == "taps_not_reversed" else -sh
        dx = dx + shift(dz_, lens, back) @ f(Wj)
        adx += shift(adz, lens, -sh) @ np.abs(Wj)
        edx += shift(e_dz, lens, -sh) @ np.abs(Wj)
        xs, axs, exs = shift(f(x), lens, sh), shift(np.abs(x).astype(np.float64), lens, sh), shift(ex, lens, sh)
        dconv[:, :, j] = dz_.T @ xs
        e_dconv[:, :, j] = (n + 2) * U * (adz.T @ axs) + e_dz.T @ axs + adz.T @ exs + e_dz.T @ exs
    if dxo is not None:
        dx = dx + f(dxo) * dt(1.0 if mutant == "no_sqrt_half_residual" else SQH)
        adx += SQH * np.abs(dxo)
        edx += SQH * edxo
    e_dx = (2 * k * R + 3) * U * adx + edx
    dc, e_dc = dz_ @ f(w["aux"]), (2 * R + 2) * U * (adz @ np.abs(w["aux"])) + e_dz @ np.abs(w["aux"])
    db_conv, e_db_conv = dz_.sum(0), (n + 2) * U * adz.sum(0) + e_dz.sum(0)
    if mutant == "missing_bias_gradient":
        db_conv = np.zeros_like(db_conv)
    ac = np.abs(c).astype(np.float64)
    daux, e_daux = dz_.T @ f(c), (n + 2) * U * (adz.T @ ac) + e_dz.T @ ac
    g = f(a) * f(b)
    ag, eg = np.abs(g).astype(np.float64), _gate_product_error(a, b, ea, eb)
    ads = np.abs(ds).astype(np.float64)
    dskip, e_dskip = f(ds).T @ g, (n + 3) * U * (ads.T @ ag) + ads.T @ eg
    db_skip, e_db_skip = f(ds).sum(0), (n + 2) * U * ads.sum(0)
    if dxo is None:
        dout, e_dout, db_out, e_db_out = np.zeros((R, R), dt), np.zeros((R, R)), np.zeros(R, dt), np.zeros(R)
    else:
        sx, asx = f(dxo) * dt(SQH), SQH * np.abs(dxo).astype(np.float64)
        dout, e_dout = sx.T @ g, (n + 4) * U * (asx.T @ ag) + SQH * (edxo.T @ ag + np.abs(dxo).T @ eg + edxo.T @ eg)
        db_out, e_db_out = sx.sum(0), (n + 3) * U * asx.sum(0) + SQH * edxo.sum(0)
    return dict(dx=dx, e_dx=e_dx, dc=dc, e_dc=e_dc,
                grads=(dconv, db_conv, daux[:, :, None], dout[:, :, None], db_out, dskip[:, :, None], db_skip),
                e_grads=(e_dconv, e_db_conv, e_daux[:, :, None], e_dout[:, :, None], e_db_out, e_dskip[:, :, None], e_db_skip))


def stack_forward(ws, x0, c, lens, dils, mutant=None, dt=np.float64, running=True):
    """-> per block dict(x (the block's input), a, b, x_out, e_x (of the input), e_a, e_b, e_xout), and skips (un-scaled), e_s: the running bounds
    (running False: every block's first term only -- over 30 saturating blocks the running bounds say nothing)"""
    x, ex, skips, es, blocks = np.asarray(x0, dt), np.zeros(x0.shape), None, None, []
    for w, d in zip(ws, dils):
        gt = gate_forward(w, x, c, lens, d, ex if running else None, mutant, dt)
        o = out_forward(w, x, gt["a"], gt["b"], skips, ex if running else None, gt["e_a"], gt["e_b"], es if running else None, dt)
        blocks.append(dict(x=x, e_x=ex, a=gt["a"], b=gt["b"], z=gt["z"], e_a=gt["e_a"], e_b=gt["e_b"], x_out=o["x_out"], e_xout=o["e_x"]))
        x, ex, skips, es = o["x_out"], o["e_x"], o["skips"], o["e_s"]
    return dict(blocks=blocks, skips=skips, e_s=es)


def stack_backward(ws, fw, c, ds, lens, dils, running=True, mutant=None, dt=np.float64):
    """on the forward pass's kept x_l, a_l, b_l -> dx0, dc, per block the seven parameter gradients, and the bounds (running: with the forward pass's and
    the earlier backward blocks' errors; else the inputs count as exact)"""
    L = len(ws)
    g, eg, dc, e_dc, grads, e_grads = None, None, None, None, [None] * L, [None] * L
    for l in range(L - 1, -1, -1):
        blk = fw["blocks"][l]
        err = dict(ex=blk["e_x"], ea=blk["e_a"], eb=blk["e_b"], edxo=eg) if running else None
        r = block_backward(ws[l], blk["x"], c, blk["a"], blk["b"], g, ds, lens, dils[l], err, mutant, dt)
        if dc is None or mutant == "dc_overwritten":
            dc, e_dc = r["dc"], r["e_dc"]
        else:
            dc = dc + r["dc"]
            e_dc = e_dc + r["e_dc"] + U * np.abs(dc)
        g, eg, grads[l], e_grads[l] = r["dx"], r["e_dx"], r["grads"], r["e_grads"]
    return dict(dx0=g, e_dx0=eg, dc=dc, e_dc=e_dc, grads=grads, e_grads=e_grads)


# ---- the cases' inputs: helpers.py's builders, which saturate the gate (asserted in test_pwg_generator_cpu.py)
def block_case(name, d, seed=900):
    """-> (weights dict, inputs dict x / c / skips / dxo / ds, float32 values) of one block-level cell"""
    import helpers as H

    R, A, k = BLOCK_CONFIGS[name]
    sd, _ = H.pwg_block_state_dict(seed + d, R, A, k)
    n = sum(LENS)
    inp = H.pwg_block_sample_inputs(seed + d, n, R, A)
    rng = np.random.RandomState(seed + d + 7)
    g = lambda *s: rng.standard_normal(s).astype(np.float32)
    return block_weights(sd, 0), dict(x=inp["x"], c=inp["feats"], skips=inp["skips"], dxo=g(n, R), ds=g(n, R))


def stack_case(cfg, seed, gain=4.0):
    """-> (state dict, per-block weights, x0, c, ds) for a packed batch of LENS samples"""
    import helpers as H

    rng = np.random.RandomState(seed)
    sd = H.pwg_random_state_dict(rng, cfg, gain)
    n, R, A = sum(LENS), cfg["residual_channels"], cfg["aux_channels"]
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    x0, c, ds = f(n, R), np.float32(2.5) * f(n, A), f(n, R)
    return sd, [block_weights(sd, l) for l in range(cfg["layers"])], x0, c, ds


def torch_statement(sd, cfg, x0, c, ds, lens):
    """oracle.pwg_oracle.generator_forward in float64 under torch autograd, utterance by utterance: x_0 enters through an identity first_conv, and the given
    gradient ds of the un-scaled skip sum through the scaled sum it returns.  -> skips (un-scaled), taps, dx0, dc, {name: gradient}"""
    import torch

    from oracle import pwg_oracle as O

    R, L = cfg["residual_channels"], cfg["layers"]
    t = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=k.startswith("conv_layers")) for k, v in sd.items()}
    t["first_conv.weight"], t["first_conv.bias"] = torch.eye(R, dtype=torch.float64).reshape(R, R, 1), torch.zeros(R, dtype=torch.float64)
    scale = math.sqrt(1.0 / L)
    out = dict(skips=[], taps=[], dx0=[], dc=[])
    off = 0
    for n in lens:
        x = torch.tensor(np.asarray(x0[off : off + n], np.float64).T[None], requires_grad=True)
        cc = torch.tensor(np.asarray(c[off : off + n], np.float64).T[None], requires_grad=True)
        _, taps, sk = O.generator_forward(t, x, cc, cfg, return_taps=True)
        (sk / scale).backward(torch.tensor(np.asarray(ds[off : off + n], np.float64).T[None]))
        out["skips"].append((sk[0].t() / scale).detach().numpy())
        out["taps"].append([tp[0].t().detach().numpy() for tp in taps])
        out["dx0"].append(x.grad[0].t().numpy())
        out["dc"].append(cc.grad[0].t().numpy())
        off += n
    res = {k: np.concatenate(v) for k, v in out.items() if k != "taps"}
    res["taps"] = [np.concatenate([u[l] for u in out["taps"]]) for l in range(L)]
    res["grads"] = {k: (np.zeros(v.shape) if v.grad is None else v.grad.numpy()) for k, v in t.items() if k.startswith("conv_layers")}
    return res
