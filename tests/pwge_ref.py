"""The two ends of the Parallel WaveGAN generator (csrc/pwg_ends.hip) restated in numpy on packed ragged batches, forward and backward,
with a running error bound beside every value (pwgt_ref.py's style; u = 2^-24).  dt = float64 is the statement, dt = float32 an evaluation that has to
stay inside the bounds (test_pwg_ends_cpu.py), and the mutants have to leave them.

Weights are in torch's orientation: win [A, A, 2 ctx + 1] (conv_in, no bias), hs[i] [2 s_i + 1], w0, b0 [R] (first_conv), W1 [R, R], b1 [R], w3 [R],
b3 [1] (last_conv_layers 1 and 3).  Rows are channel-last and packed: utterance b has frames[b] frames, frames[b] + 2 ctx rows of c and frames[b] hop
samples.

Bounds: a linear term of K products gets (K + 2) u sum |w| |x| plus its inputs' errors carried through |w|; a sum over n samples gets (n + 2) u sum
|.| |.|, whatever the order.  There is no transcendental.  The forward ReLUs are 1-Lipschitz and need nothing; the two backward masks have a kink: a
cell whose float64 pre-activation is no larger than its own bound may come out either way, is left out of the comparison of the array the mask stands
in (`free`), and enters what is summed from it with the whole jump as its error.  At most MAX_FREE of an array's cells may be free."""
import math

import numpy as np

U = 2.0 ** -24
MAX_FREE = 0.01
FRAMES_A, SCALES_A = (1, 2, 5, 9, 200), (2, 3)  # hop 6 (a scale that is no power of two); 1302 samples: no multiple of 128, across one 1024-sample
#                                                 chunk; the 1-frame utterance has every filter hanging over both edges, a neighbour on each side
FRAMES_B, SCALES_B = (1, 3), (4, 4, 4, 4)
MUTANTS = ("across_edge", "stretch_off_by_one", "taps_reversed_bwd", "context_offset_dropped", "no_sigma_in_ds", "s_mask_dropped", "db3_missing",
           "dh_one_channel")


def spans(frames, per=1, extra=0):
    out, off = [], 0
    for f in frames:
        out.append((off, off + f * per + extra))
        off += f * per + extra
    return out


def _z(e, like):
    return np.zeros(np.shape(like)) if e is None else e


def _abs(v):
    return np.abs(np.asarray(v, np.float64))


# ---- input side ----------------------------------------------------------------------------------------------------------------------------------
def conv_in(c, win, frames, ctx, ec=None, mutant=None, dt=np.float64):
    """u0[f] = sum_j c_b[f + j] Win_j -> dict(u, e)"""
    A, K, F = win.shape[0], 2 * ctx + 1, sum(frames)
    u, mag, ein = np.zeros((F, A), dt), np.zeros((F, A)), np.zeros((F, A))
    cc, ec = np.asarray(c, dt), _z(ec, c)
    for (lo, hi), (clo, _) in zip(spans(frames), spans(frames, extra=2 * ctx)):
        if mutant == "context_offset_dropped":
            clo = lo  # (the pack read as if no utterance had context rows)
        for j in range(K):
            Wj = win[:, :, j].T
            u[lo:hi] += cc[clo + j : clo + j + hi - lo] @ np.asarray(Wj, dt)
            mag[lo:hi] += _abs(cc[clo + j : clo + j + hi - lo]) @ _abs(Wj)
            ein[lo:hi] += ec[clo + j : clo + j + hi - lo] @ _abs(Wj)
    return dict(u=u, e=(K * A + 2) * U * mag + ein)


def _taps(n_in, s, mutant=None):
    """for one utterance of n_in input rows: per tap j (ok [n_out] bool, idx [n_out] the input row read)"""
    t = np.arange(n_in * s)
    for j in range(2 * s + 1):
        p = t + j - s
        yield j, (p >= 0) & (p < n_in * s), np.clip((p + (1 if mutant == "stretch_off_by_one" else 0)) // s, 0, n_in - 1)


def stage(u, h, rows, s, eu=None, mutant=None, dt=np.float64):
    """rows: the input rows of every utterance.  out[t] = sum_j h[j] u[(t + j - s) div s] inside the utterance -> dict(u, e)"""
    A, n_all = u.shape[1], sum(rows)
    out, mag, ein = np.zeros((n_all * s, A), dt), np.zeros((n_all * s, A)), np.zeros((n_all * s, A))
    uu, eu, off = np.asarray(u, dt), _z(eu, u), 0
    for n in ([n_all] if mutant == "across_edge" else rows):
        sl = slice(off * s, (off + n) * s)
        for j, ok, idx in _taps(n, s, mutant):
            out[sl] += dt(h[j]) * np.where(ok[:, None], uu[off:off + n][idx], dt(0))
            mag[sl] += abs(float(h[j])) * np.where(ok[:, None], _abs(uu[off:off + n][idx]), 0.0)
            ein[sl] += abs(float(h[j])) * np.where(ok[:, None], eu[off:off + n][idx], 0.0)
        off += n
    return dict(u=out, e=(2 * s + 3) * U * mag + ein)


def stage_backward(g, h, rows, s, eg=None, mutant=None, dt=np.float64):
    """the transposed stretch and filter: g [n s, A] -> du [n, A] -> dict(d, e)"""
    A, n_all = g.shape[1], sum(rows)
    gg, eg, off = np.asarray(g, dt), _z(eg, g), 0
    du, mag, ein = np.zeros((n_all, A), dt), np.zeros((n_all, A)), np.zeros((n_all, A))
    for n in rows:
        gb, eb = gg[off * s : (off + n) * s], eg[off * s : (off + n) * s]
        d, m, e = np.zeros((n * s, A), dt), np.zeros((n * s, A)), np.zeros((n * s, A))
        t = np.arange(n * s)
        for j, ok, _ in _taps(n, s):
            hj = h[2 * s - j] if mutant == "taps_reversed_bwd" else h[j]
            p = t[ok] + j - s
            d[p] += dt(hj) * gb[ok]
            m[p] += abs(float(hj)) * _abs(gb[ok])
            e[p] += abs(float(hj)) * eb[ok]
        du[off:off + n], mag[off:off + n], ein[off:off + n] = (v.reshape(n, s, A).sum(1) for v in (d, m, e))
        off += n
    return dict(d=du, e=(s * (2 * s + 1) + 2) * U * mag + ein)


def filter_gradient(u, g, rows, s, eu=None, eg=None, mutant=None, dt=np.float64):
    """dh[j] = sum_{t, a} u[(t + j - s) div s, a] g[t, a] -> dict(d, e)"""
    A = 1 if mutant == "dh_one_channel" else u.shape[1]
    uu, gg, eu, eg, off = np.asarray(u, dt), np.asarray(g, dt), _z(eu, u), _z(eg, g), 0
    dh, mag, ein = np.zeros(2 * s + 1, dt), np.zeros(2 * s + 1), np.zeros(2 * s + 1)
    for n in rows:
        gb, egb = gg[off * s : (off + n) * s, :A], eg[off * s : (off + n) * s, :A]
        for j, ok, idx in _taps(n, s):
            term, et = np.where(ok[:, None], uu[off:off + n][idx], dt(0))[:, :A], np.where(ok[:, None], eu[off:off + n][idx], 0.0)[:, :A]
            dh[j] += (term * gb).sum(dtype=dt)
            mag[j] += (_abs(term) * _abs(gb)).sum()
            ein[j] += (_abs(term) * egb + et * _abs(gb) + et * egb).sum()
        off += n
    return dict(d=dh, e=(sum(rows) * s * u.shape[1] + 2) * U * mag + ein)


def conv_in_backward(c, du0, win, frames, ctx, edu=None, dt=np.float64):
    """-> dict(dwin [A, A, K], e_dwin, dc [rows of c, A], e_dc)"""
    A, K = win.shape[0], 2 * ctx + 1
    cc, dd, edu = np.asarray(c, dt), np.asarray(du0, dt), _z(edu, du0)
    dwin, mw, ew = np.zeros(win.shape, dt), np.zeros(win.shape), np.zeros(win.shape)
    dc, mc, ecc = np.zeros(cc.shape, dt), np.zeros(cc.shape), np.zeros(cc.shape)
    for (lo, hi), (clo, _) in zip(spans(frames), spans(frames, extra=2 * ctx)):
        for j in range(K):
            rows = slice(clo + j, clo + j + hi - lo)
            dwin[:, :, j] += dd[lo:hi].T @ cc[rows]
            mw[:, :, j] += _abs(dd[lo:hi]).T @ _abs(cc[rows])
            ew[:, :, j] += edu[lo:hi].T @ _abs(cc[rows])
            dc[rows] += dd[lo:hi] @ np.asarray(win[:, :, j], dt)
            mc[rows] += _abs(dd[lo:hi]) @ _abs(win[:, :, j])
            ecc[rows] += edu[lo:hi] @ _abs(win[:, :, j])
    return dict(dwin=dwin, e_dwin=(sum(frames) + 2) * U * mw + ew, dc=dc, e_dc=(K * A + 2) * U * mc + ecc)


def first_conv(z, w0, b0, dt=np.float64):
    x0 = np.asarray(z, dt)[:, None] * np.asarray(w0, dt) + np.asarray(b0, dt)
    return dict(x0=x0, e=2 * U * (_abs(z)[:, None] * _abs(w0) + _abs(b0)))


def first_conv_backward(z, dx0, w0, edx=None, dt=np.float64):
    zz, dd, edx, n = np.asarray(z, dt), np.asarray(dx0, dt), _z(edx, dx0), len(z)
    return dict(dw0=(zz[:, None] * dd).sum(0, dtype=dt), e_dw0=(n + 2) * U * (_abs(zz)[:, None] * _abs(dd)).sum(0) + (_abs(zz)[:, None] * edx).sum(0),
                db0=dd.sum(0, dtype=dt), e_db0=(n + 2) * U * _abs(dd).sum(0) + edx.sum(0),
                dz=dd @ np.asarray(w0, dt), e_dz=(len(w0) + 2) * U * (_abs(dd) @ _abs(w0)) + edx @ _abs(w0))


def stage_rows(frames, scales):
    """per stage the input rows of every utterance"""
    out, rows = [], list(frames)
    for s in scales:
        out.append(rows)
        rows = [r * s for r in rows]
    return out


def input_forward(w, c, z, frames, scales, ctx, mutant=None, dt=np.float64, running=True):
    """-> dict(us [u_0 .. u_{n-1}], e_us, cu, e_cu, x0, e_x0); running False: every launch on the previous one's values as exact inputs"""
    r = conv_in(c, w["win"], frames, ctx, None, mutant, dt)
    us, e_us = [r["u"]], [r["e"]]
    for i, (s, rows) in enumerate(zip(scales, stage_rows(frames, scales))):
        r = stage(us[-1], w["hs"][i], rows, s, e_us[-1] if running else None, mutant, dt)
        us.append(r["u"])
        e_us.append(r["e"])
    f = first_conv(z, w["w0"], w["b0"], dt)
    return dict(us=us[:-1], e_us=e_us[:-1], cu=us[-1], e_cu=e_us[-1], x0=f["x0"], e_x0=f["e"])


def input_backward(w, c, z, fw, dcu, dx0, frames, scales, ctx, mutant=None, dt=np.float64, running=True, e_dcu=None, e_dx0=None):
    """on the forward pass's kept u_i -> dict(dus [du_0 ..], e_dus, dhs, e_dhs, dwin, e_dwin, dc, e_dc, dw0, e_dw0, db0, e_db0, dz, e_dz); e_dcu, e_dx0:
    the errors the incoming gradients arrive with (the whole generator)"""
    g, eg, dus, e_dus, dhs, e_dhs = dcu, e_dcu, [], [], [], []
    all_rows = stage_rows(frames, scales)
    for i in range(len(scales) - 1, -1, -1):
        s, rows = scales[i], all_rows[i]
        h = filter_gradient(fw["us"][i], g, rows, s, fw["e_us"][i] if running else None, eg if running else None, mutant, dt)
        b = stage_backward(g, w["hs"][i], rows, s, eg if running else None, mutant, dt)
        dhs.insert(0, h["d"])
        e_dhs.insert(0, h["e"])
        dus.insert(0, b["d"])
        e_dus.insert(0, b["e"])
        g, eg = b["d"], b["e"]
    out = conv_in_backward(c, g, w["win"], frames, ctx, eg if running else None, dt)
    out.update(first_conv_backward(z, dx0, w["w0"], e_dx0, dt))
    out.update(dus=dus, e_dus=e_dus, dhs=dhs, e_dhs=e_dhs)
    return out


# ---- output side ---------------------------------------------------------------------------------------------------------------------------------
def output_forward(w, S, layers, eS=None, dt=np.float64):
    """-> dict(v, e_v, p1 (the pre-activation of y1), y1, e_y1, wav, e_wav)"""
    sig, R = math.sqrt(1.0 / layers), S.shape[1]
    SS, eS = np.asarray(S, dt), _z(eS, S)
    pre = dt(sig) * SS
    v, e_v = np.maximum(pre, dt(0)), 2 * U * _abs(pre) + sig * eS
    W1t = np.asarray(w["W1"], dt).T
    p1 = v @ W1t + np.asarray(w["b1"], dt)
    e_p1 = (R + 2) * U * (_abs(v) @ _abs(W1t) + _abs(w["b1"])) + e_v @ _abs(W1t)
    y1 = np.maximum(p1, dt(0))
    wav = y1 @ np.asarray(w["w3"], dt) + dt(np.asarray(w["b3"]).reshape(-1)[0])
    e_wav = (R + 2) * U * (_abs(y1) @ _abs(w["w3"]) + abs(float(np.asarray(w["b3"]).reshape(-1)[0]))) + e_p1 @ _abs(w["w3"])
    return dict(pre=pre, v=v, e_v=e_v, e_pre=2 * U * _abs(pre) + sig * eS, p1=p1, e_p1=e_p1, y1=y1, e_y1=e_p1, wav=wav, e_wav=e_wav)


def output_backward(w, S, layers, dwav, on1, ons, free1=None, frees=None, e_v=None, e_y1=None, y1=None, dy1=None, mutant=None, dt=np.float64):
    """on1 / ons: the masks [y1 > 0] and [sigma S > 0] (bool); free1 / frees: their cells that may come out either way.  y1: the kept activation (None:
    no dw3).  dy1: a given dy1, taken as exact (a launch alone on the device's own inputs) ->
    dict(dy1, e_dy1, ds, e_ds, dW1 [out, in], e_dW1, db1, e_db1, dw3, e_dw3, db3, e_db3)"""
    sig, R, n = math.sqrt(1.0 / layers), S.shape[1], len(S)
    g, w3, W1 = np.asarray(dwav, dt), np.asarray(w["w3"], dt), np.asarray(w["W1"], dt)
    full = g[:, None] * w3
    if dy1 is None:
        d1 = np.where(on1, full, dt(0))
        e_d1 = U * _abs(d1) + (0.0 if free1 is None else np.where(free1, _abs(full), 0.0))
    else:
        d1, e_d1 = np.asarray(dy1, dt), np.zeros(S.shape)
    lin = d1 @ W1
    keep = np.ones(S.shape, bool) if mutant == "s_mask_dropped" else ons
    ds = np.where(keep, (dt(1) if mutant == "no_sigma_in_ds" else dt(sig)) * lin, dt(0))
    e_lin = (R + 3) * U * (_abs(d1) @ _abs(W1)) + e_d1 @ _abs(W1)
    e_ds = np.where(ons, sig * e_lin, 0.0) + (0.0 if frees is None else np.where(frees, sig * (_abs(lin) + e_lin), 0.0))
    v = np.maximum(dt(sig) * np.asarray(S, dt), dt(0))
    e_v = 2 * U * _abs(v) if e_v is None else e_v
    out = dict(dy1=d1, e_dy1=e_d1, ds=ds, e_ds=e_ds)
    out["dW1"] = d1.T @ v
    out["e_dW1"] = (n + 2) * U * (_abs(d1).T @ _abs(v)) + e_d1.T @ _abs(v) + _abs(d1).T @ e_v + e_d1.T @ e_v
    out["db1"], out["e_db1"] = d1.sum(0, dtype=dt), (n + 2) * U * _abs(d1).sum(0) + e_d1.sum(0)
    if y1 is not None:
        yy, e_y1 = np.asarray(y1, dt), _z(e_y1, y1)
        out["dw3"], out["e_dw3"] = (g[:, None] * yy).sum(0, dtype=dt), (n + 2) * U * (_abs(g)[:, None] * _abs(yy)).sum(0) + (_abs(g)[:, None] * e_y1).sum(0)
    out["db3"] = np.zeros(1, dt) if mutant == "db3_missing" else g.sum(dtype=dt).reshape(1)
    out["e_db3"] = (n + 2) * U * _abs(g).sum().reshape(1)
    return out


def output_end(w, S, layers, dwav, mutant=None, dt=np.float64):
    """the output side end to end with its running bound: forward, then backward on the forward's own masks.  -> (forward dict, backward dict, free
    dict(y1, s): the cells left out of the comparisons of dy1 and ds)"""
    fw = output_forward(w, S, layers, None, dt)
    free1 = np.abs(fw["p1"]) <= fw["e_p1"]
    frees = np.zeros(S.shape, bool)  # (S is this end's input: sigma S > 0 is decided by the sign of S)
    bw = output_backward(w, S, layers, dwav, fw["p1"] > 0, np.asarray(S) > 0, free1, frees, fw["e_v"], fw["e_y1"], fw["y1"], None, mutant, dt)
    return fw, bw, dict(y1=free1, s=frees)


# ---- the cases' inputs ------------------------------------------------------------------------------------------------------------------------------
def end_weights(seed, R, A, ctx, scales):
    """unit-scale weights in torch's orientation (float32 values); the stage filters near their initial 1 / (2 s + 1)"""
    rng = np.random.RandomState(seed)
    g = lambda *s: rng.standard_normal(s).astype(np.float32)
    K = 2 * ctx + 1
    return dict(win=g(A, A, K) / np.float32(math.sqrt(K * A)), hs=[(np.float32(1.0 / (2 * s + 1)) * (1 + np.float32(0.5) * g(2 * s + 1))).astype(np.float32) for s in scales],
                w0=g(R), b0=np.float32(0.1) * g(R), W1=g(R, R) / np.float32(math.sqrt(R)), b1=np.float32(0.1) * g(R), w3=g(R) / np.float32(math.sqrt(R)),
                b3=np.float32(0.1) * g(1))


def end_case(seed, frames, scales, R, A, ctx):
    """-> (weights, inputs dict c / z / dcu / dx0 / S / dwav, float32) for a packed batch"""
    rng = np.random.RandomState(seed + 1)
    g = lambda *s: rng.standard_normal(s).astype(np.float32)
    n = sum(frames) * int(np.prod(scales))
    return end_weights(seed, R, A, ctx, scales), dict(c=g(sum(frames) + 2 * ctx * len(frames), A), z=g(n), dcu=g(n, A), dx0=g(n, R), S=np.float32(3.0) * g(n, R),
                                                    dwav=g(n))


def state_dict_of(w, R, A):
    """the ends' weights under the reference's names (plain, no weight norm), float64"""
    sd = {"upsample_net.conv_in.weight": w["win"], "first_conv.weight": np.asarray(w["w0"]).reshape(R, 1, 1), "first_conv.bias": w["b0"],
          "last_conv_layers.1.weight": np.asarray(w["W1"]).reshape(R, R, 1), "last_conv_layers.1.bias": w["b1"],
          "last_conv_layers.3.weight": np.asarray(w["w3"]).reshape(1, R, 1), "last_conv_layers.3.bias": np.asarray(w["b3"]).reshape(1)}
    for i, h in enumerate(w["hs"]):
        sd["upsample_net.upsample.up_layers.%d.weight" % (2 * i + 1)] = np.asarray(h).reshape(1, 1, 1, -1)
    return {k: np.asarray(v, np.float64) for k, v in sd.items()}


def weights_of(sd, n_scales):
    """the inverse of state_dict_of on a whole generator's plain state dict"""
    f = lambda k: np.asarray(sd[k])
    return dict(win=f("upsample_net.conv_in.weight"), hs=[f("upsample_net.upsample.up_layers.%d.weight" % (2 * i + 1)).reshape(-1) for i in range(n_scales)],
                w0=f("first_conv.weight").reshape(-1), b0=f("first_conv.bias"), W1=f("last_conv_layers.1.weight")[:, :, 0], b1=f("last_conv_layers.1.bias"),
                w3=f("last_conv_layers.3.weight").reshape(-1), b3=f("last_conv_layers.3.bias").reshape(1))


SHAPES = {"hop6": (FRAMES_A, SCALES_A), "hop256": (FRAMES_B, SCALES_B)}
LAYERS = 4  # sigma = 1 / 2
CASES = [(shape, A, ctx, R) for shape in SHAPES for A in (16, 80) for ctx in (0, 2) for R in (16, 64)]
_cache = {}


def reference(shape, A, ctx, R):
    """one case's float32 inputs and its float64 statement with the running bounds, computed once and shared (read-only): dict(w, inp, frames, scales,
    fw, bw (input side), ofw, obw, free (output side))"""
    key = (shape, A, ctx, R)
    if key not in _cache:
        frames, scales = SHAPES[shape]
        w, inp = end_case(500 + 7 * A + ctx + R, frames, scales, R, A, ctx)
        fw = input_forward(w, inp["c"], inp["z"], frames, scales, ctx)
        bw = input_backward(w, inp["c"], inp["z"], fw, inp["dcu"], inp["dx0"], frames, scales, ctx)
        ofw, obw, free = output_end(w, inp["S"], LAYERS, inp["dwav"])
        for v in list(w.values()) + list(inp.values()):
            for a in (v if isinstance(v, list) else [v]):
                a.setflags(write=False)
        _cache[key] = dict(w=w, inp=inp, frames=frames, scales=scales, fw=fw, bw=bw, ofw=ofw, obw=obw, free=free)
    return _cache[key]


def share(diff, bound, free=None):
    """the worst |diff| / bound over the cells that are not free; a bound of exactly zero admits exactly zero"""
    r = np.abs(diff) / np.maximum(bound, 1e-300)
    return float(np.max(r if free is None else np.where(free, 0.0, r)))


# ---- the whole generator: the ends around pwgt_ref's residual stack, with every error carried from (z, c) to the waveform and back -------------------------
def generator(sd, cfg, c, z, dwav, frames):
    """float64 values and running float32 bounds of the waveform and of every parameter's gradient (torch's names and orientation) for a packed batch.
    pwgt_ref's block functions carry the errors of x, a, b and dxo; the conditioning's error (the input side's e_cu) and the error ds arrives with
    (the output side's e_ds) are carried here, term by term: e_cu |Waux| into the gate (tanh is 1-Lipschitz, the sigmoid 1/4), e_ds |Wskip| into dg
    and from there through |b (1 - a^2)| <= 1, |a b (1 - b)| <= 1/4 (with room for their own rounding) into dz and everything summed from dz, and
    e_ds straight into the skip convolution's gradients.  A cell of a backward mask that may come out either way carries its whole jump.
    -> (wav, e_wav, {name: gradient}, {name: bound})"""
    import pwgt_ref as R

    scales, ctx, L = tuple(cfg["upsample_scales"]), cfg["aux_context_window"], cfg["layers"]
    hop, Rc = int(np.prod(scales)), cfg["residual_channels"]
    lens, dils = [f * hop for f in frames], R.dilations(cfg)
    w, ws = weights_of(sd, len(scales)), [R.block_weights(sd, l) for l in range(L)]
    fi = input_forward(w, c, z, frames, scales, ctx)
    cu, e_cu = fi["cu"], fi["e_cu"]
    x, ex, skips, es, blocks = fi["x0"], fi["e_x0"], None, None, []
    for wl, d in zip(ws, dils):
        gt = R.gate_forward(wl, x, cu, lens, d, ex)
        more = e_cu @ np.abs(wl["aux"].T)
        ea, eb = gt["e_a"] + more[:, :Rc], gt["e_b"] + more[:, Rc:] / 4
        o = R.out_forward(wl, x, gt["a"], gt["b"], skips, ex, ea, eb, es)
        blocks.append(dict(x=x, ex=ex, a=gt["a"], b=gt["b"], ea=ea, eb=eb))
        x, ex, skips, es = o["x_out"], o["e_x"], o["skips"], o["e_s"]
    fo = output_forward(w, skips, L, es)
    free1, frees = np.abs(fo["p1"]) <= fo["e_p1"], np.abs(fo["pre"]) <= fo["e_pre"]
    bo = output_backward(w, skips, L, dwav, fo["p1"] > 0, skips > 0, free1, frees, fo["e_v"], fo["e_y1"], fo["y1"])
    ds, eds = bo["ds"], bo["e_ds"]
    grads = {"last_conv_layers.1.weight": bo["dW1"][:, :, None], "last_conv_layers.1.bias": bo["db1"], "last_conv_layers.3.weight": bo["dw3"][None, :, None],
             "last_conv_layers.3.bias": bo["db3"]}
    bounds = {"last_conv_layers.1.weight": bo["e_dW1"][:, :, None], "last_conv_layers.1.bias": bo["e_db1"],
              "last_conv_layers.3.weight": bo["e_dw3"][None, :, None], "last_conv_layers.3.bias": bo["e_db3"]}
    g, eg, dc, e_dc = None, None, None, None
    for l in range(L - 1, -1, -1):
        wl, blk, d = ws[l], blocks[l], dils[l]
        r = R.block_backward(wl, blk["x"], cu, blk["a"], blk["b"], g, ds, lens, d, dict(ex=blk["ex"], ea=blk["ea"], eb=blk["eb"], edxo=eg))
        k = wl["conv"].shape[2]
        m_dg = eds @ np.abs(wl["skip"])
        m_dz = np.concatenate([1.0001 * m_dg, 0.2501 * m_dg], axis=1)
        adz, e_dz = np.abs(r["dz"]), r["e_dz"]
        m_dx, m_conv = np.zeros(blk["x"].shape), np.zeros(wl["conv"].shape)
        for j in range(k):
            sh = (j - (k - 1) // 2) * d
            m_dx += R.shift(m_dz, lens, -sh) @ np.abs(wl["conv"][:, :, j])
            m_conv[:, :, j] = m_dz.T @ (R.shift(np.abs(blk["x"]), lens, sh) + R.shift(blk["ex"], lens, sh))
        m_aux = m_dz.T @ (np.abs(cu) + e_cu) + (adz + e_dz).T @ e_cu
        gp, egp = np.abs(blk["a"] * blk["b"]), R._gate_product_error(blk["a"], blk["b"], blk["ea"], blk["eb"])
        more = (m_conv, m_dz.sum(0), m_aux[:, :, None], 0.0, 0.0, (eds.T @ (gp + egp))[:, :, None], eds.sum(0))
        for name, val, e, m in zip(("conv.weight", "conv.bias", "conv1x1_aux.weight", "conv1x1_out.weight", "conv1x1_out.bias", "conv1x1_skip.weight",
                                    "conv1x1_skip.bias"), r["grads"], r["e_grads"], more):
            grads["conv_layers.%d.%s" % (l, name)], bounds["conv_layers.%d.%s" % (l, name)] = val, e + m
        this_dc, this_e = r["dc"], r["e_dc"] + m_dz @ np.abs(wl["aux"])
        dc, e_dc = (this_dc, this_e) if dc is None else (dc + this_dc, e_dc + this_e + U * np.abs(dc + this_dc))
        g, eg = r["dx"], r["e_dx"] + m_dx
    bi = input_backward(w, c, z, fi, dc, g, frames, scales, ctx, e_dcu=e_dc, e_dx0=eg)
    grads.update({"upsample_net.conv_in.weight": bi["dwin"], "first_conv.weight": bi["dw0"][:, None, None], "first_conv.bias": bi["db0"]})
    bounds.update({"upsample_net.conv_in.weight": bi["e_dwin"], "first_conv.weight": bi["e_dw0"][:, None, None], "first_conv.bias": bi["e_db0"]})
    for i in range(len(scales)):
        name = "upsample_net.upsample.up_layers.%d.weight" % (2 * i + 1)
        grads[name], bounds[name] = bi["dhs"][i].reshape(1, 1, 1, -1), bi["e_dhs"][i].reshape(1, 1, 1, -1)
    return fo["wav"], fo["e_wav"], grads, bounds


MODULE_FRAMES = (1, 5, 22)


def module_case():
    """the module-level comparison's case, shared by the CPU and the GPU test: (cfg, state dict (float32), mels, noise, dwav [samples]) at hop 6, a
    2-block stack and weights at a quarter of helpers' gain -- the running bound grows with the absolute row sums of every matrix on the way, and at 4
    blocks and full gain it exceeds the waveform's peak and says nothing; test_pwg_ends_cpu.py asserts that here it stays under 1e-2 of the peak"""
    import helpers as H
    import pwgt_ref as R

    cfg = dict(H.pwg_cfg(dict(R.SMALL_STACK, layers=2, stacks=1, upsample_scales=(2, 3))))
    sd, mels, noise = H.pwg_generator_inputs(47, list(MODULE_FRAMES), cfg, gain=0.25)
    dwav = np.random.RandomState(3).standard_normal(sum(MODULE_FRAMES) * 6).astype(np.float32)
    return cfg, sd, mels, noise, dwav


def module_reference():
    """-> (cp, zp (the packed inputs), wav, e_wav, grads, bounds) of module_case, computed once"""
    if "module" not in _cache:
        cfg, sd, mels, noise, dwav = module_case()
        ctx = cfg["aux_context_window"]
        cp = np.concatenate([m[np.clip(np.arange(-ctx, len(m) + ctx), 0, len(m) - 1)] for m in mels])
        zp = np.concatenate(noise)
        _cache["module"] = (cp, zp) + generator({k: np.asarray(v, np.float64) for k, v in sd.items()}, cfg, cp, zp, dwav, list(MODULE_FRAMES))
    return _cache["module"]


# ---- the STFT loss of a waveform that is known to within e: what the driver's step 1 may differ by between two float32 evaluations ------------------
def stft_loss_bounds(x, e, y, resolutions):
    """x [B, n] the float64 statement's waveforms, e [B, n] their elementwise float32 bounds (generator), y [B, n] the targets (exact), equal lengths,
    reduction "batch" -> (sc, mag, e_sc, e_mag) with stft_loss_ref's statement and its kernel bounds (mag_delta, SUM_U), and the input's error carried
    without linearising, so that a bound as large as the signal still holds:
      per frame ||d m_x||_2 <= ||d X||_2 <= sqrt(n_fft) ||w e_frame||_2 (Parseval; |.| and the clamp are 1-Lipschitz) + mag_delta;
      a = sqrt(A), b = sqrt(B) move by at most D = ||(d_x + d_y)_frames||_2 and D_y, so sc = a / b stays in [max(a - D, 0) / (b + D_y), (a + D) / (b - D_y)];
      a bin's |log m' - log m| <= log(m / max(m - d, m_0)) with d the frame's bound and m_0 the clamp's floor (the larger of the two one-sided terms);
      plus stft_loss_ref's roundings of the float32 sums and of logf."""
    import stft_loss_ref as S

    scs, mags, e_scs, e_mags = [], [], [], []
    m0 = math.sqrt(S.CLAMP) * (1 - 4 * U)
    for case in resolutions:
        n_fft, hop, _ = case
        w = S.window(case)
        A = B = C = D2 = Dy2 = eC = 0.0
        n = 0
        for xb, eb, yb in zip(x, e, y):
            X, Y = S.spectrum(xb, w, hop), S.spectrum(yb, w, hop)
            mx, my = S.magnitudes(X), S.magnitudes(Y)
            idx = S.frame_index(len(xb), n_fft, hop)
            dx = math.sqrt(n_fft) * np.linalg.norm(np.asarray(eb, np.float64)[idx] * w, axis=1) + S.mag_delta(X, n_fft)
            dy = S.mag_delta(Y, n_fft)
            fs = S.frame_sums(xb, yb, w, hop)
            A, B, C, n = A + fs[:, 0].sum(), B + fs[:, 1].sum(), C + fs[:, 2].sum(), n + mx.size
            D2, Dy2 = D2 + ((dx + dy) ** 2).sum(), Dy2 + (dy ** 2).sum()
            eC += (np.log(mx / np.maximum(mx - dx[:, None], m0)) + np.log(my / np.maximum(my - dy[:, None], m0))).sum()
            eC += 4 * U * (np.maximum(1, np.abs(np.log(mx))) + np.maximum(1, np.abs(np.log(my)))).sum()
        a, b, D, Dy = math.sqrt(A), math.sqrt(B), math.sqrt(D2), math.sqrt(Dy2)
        assert Dy < b / 2
        rel = (S.SUM_U + 8) * U
        hi, lo = (a + D) / (b - Dy) * (1 + rel), max(a - D, 0.0) / (b + Dy) * (1 - rel)
        scs.append(a / b)
        e_scs.append(max(hi - a / b, a / b - lo))
        mags.append(C / n)
        e_mags.append((eC + (S.SUM_U + 6) * U * (C + eC)) / n)
    return float(np.mean(scs)), float(np.mean(mags)), float(np.mean(e_scs)), float(np.mean(e_mags))
