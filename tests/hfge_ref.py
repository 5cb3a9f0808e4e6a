"""Float64 numpy statement of the HiFi-GAN generator's output end -- LeakyReLU at hifigan.OUT_SLOPE, output_conv, tanh -- forward and backward on packed
rows, with derived worst-case bounds (the contract of include/fcl_hip.h "HiFi-GAN generator, output end").  Built on hfgt_ref's shift /
lrelu / mask / masked / share: arrays are packed [rows, C] with the utterance lengths `lens`, the weight is in torch's orientation (cout, C, k).

Bounds, u = 2^-24, in hfgt_ref's style.  The pre-activation is a contraction of K = k C products: (K + 3) u sum |w| |l(x)| (the LeakyReLU product on
load, the lanes' partial sums, the bias) plus |w| e_x.  tanh is 1-Lipschitz: e_wav = e_pre + E_TANH u.  dpre = dwav (1 - wav^2): wav^2 and the
subtraction each round once (2 u, both operands at most 1), the product once, and an error of wav enters as 2 |wav| e_wav + e_wav^2.  The input gradient
is a contraction of k cout products of dpre, then the mask m(x) by hfgt_ref.masked's unsure-cell rule (with exact x no cell is unsure).  The weight and
bias gradients are sums over n rows: (n + 2) u sum |.| |.| plus the operands' errors.

E_TANH is the one constant that is measured and not derived: the device library's tanhf against float64 np.tanh.  Measured through fcl_hfe_fwd's own
output on C = 16, k = 3 with ONE nonzero weight (the pre-activation is one product and a zero bias: e_pre = 2 u |pre| is known and subtracted), the
pre-activations sweeping [-9, 9] on 1 000 000 points: see E_TANH_OBSERVED below.  The constant is twice the worst observed value, because a grid can
miss the worst argument."""
import numpy as np

from hfgt_ref import LENS, MASK_CAP, SLOPE as STAGE_SLOPE, U, _z, a64, lrelu, masked, share, shift  # noqa: F401

OUT_SLOPE = float(np.float32(0.01))  # float32(hifigan.OUT_SLOPE): the slope the device multiplies by
# units of u: the worst |wav - tanh(pre)| - e_pre over the sweep, on an MI355X on 2026-10-21 (at pre = -0.6455; the worst |wav - tanh(pre)| itself,
# with nothing subtracted, was 1.8465 u)
E_TANH_OBSERVED = 0.5555
E_TANH = 2 * E_TANH_OBSERVED
TORCH_E_TANH = 4.0  # torch's tanh on the device, as pwgt_ref.E_T (measured there)
CELLS = [(16, 1, 3), (32, 1, 7), (32, 2, 5), (256, 4, 11), (64, 3, 7)]  # (C, cout, k)
MUTANTS = ("taps_not_reversed", "mask_dropped", "tanh_prime_dropped", "tanh_prime_abs", "tap_across_edge", "missing_bias_gradient", "stage_slope")


def _slope(slope, mutant):
    return STAGE_SLOPE if mutant == "stage_slope" else slope


def end_pre(x, w, b, lens, slope=OUT_SLOPE, ex=None, mutant=None, dt=np.float64):
    """pre[t, o] = b[o] + sum_j sum_ch l(x)[t + j - h, ch] W[o, ch, j] -> (pre, e_pre)"""
    f = lambda v: np.asarray(v, dtype=dt)
    k, cin = w.shape[2], w.shape[1]
    a = lrelu(f(x), _slope(slope, mutant))
    y, ay, ein = np.tile(f(b), (len(x), 1)), np.tile(a64(b), (len(x), 1)), np.zeros((len(x), w.shape[0]))
    for j in range(k):
        sh, Wj = j - (k - 1) // 2, w[:, :, j].T
        y = y + shift(a, lens, sh, mutant == "tap_across_edge") @ f(Wj)
        ay += shift(a64(a), lens, sh) @ a64(Wj)
        if ex is not None:
            ein += shift(ex, lens, sh) @ a64(Wj)
    return y, (k * cin + 3) * U * ay + ein


def end_fwd(x, w, b, lens, slope=OUT_SLOPE, ex=None, mutant=None, dt=np.float64, e_tanh=None):
    """-> (wav, e_wav); e_tanh in units of u (None: E_TANH, which must have been measured)"""
    e_tanh = E_TANH if e_tanh is None else e_tanh
    assert e_tanh is not None, "E_TANH is not measured: no forward bound"
    pre, e_pre = end_pre(x, w, b, lens, slope, ex, mutant, dt)
    return np.tanh(pre), e_pre + e_tanh * U


def dpre(wav, dwav, ewav=None, edwav=None, mutant=None, dt=np.float64):
    """dwav (1 - wav^2) -> (d, e_d)"""
    f = lambda v: np.asarray(v, dtype=dt)
    wv, g = f(wav), f(dwav)
    if mutant == "tanh_prime_dropped":
        t = np.ones_like(wv)
    elif mutant == "tanh_prime_abs":
        t = dt(1.0) - np.abs(wv)
    else:
        t = dt(1.0) - wv * wv
    d = g * t
    ew = _z(ewav, wav)
    e_t = 2 * U + 2 * a64(wav) * ew + ew * ew
    return d, a64(g) * e_t + (a64(t) + e_t) * _z(edwav, dwav) + U * a64(d)


def end_dx(x, w, wav, dwav, lens, slope=OUT_SLOPE, ex=None, ewav=None, edwav=None, mutant=None, dt=np.float64):
    """dx[t, ch] = m(x[t, ch]) sum_j sum_o dpre[t - (j - h), o] W[o, ch, j] -> (dx, e_dx, share of unsure mask cells)"""
    f = lambda v: np.asarray(v, dtype=dt)
    k, cout, cin = w.shape[2], w.shape[0], w.shape[1]
    d, e_d = dpre(wav, dwav, ewav, edwav, mutant, dt)
    across = mutant == "tap_across_edge"
    S, aS, eS = np.zeros((len(d), cin), dt), np.zeros((len(d), cin)), np.zeros((len(d), cin))
    for j in range(k):
        sh, Wj = j - (k - 1) // 2, w[:, :, j]
        S = S + shift(d, lens, sh if mutant == "taps_not_reversed" else -sh, across) @ f(Wj)
        aS += shift(a64(d), lens, -sh) @ a64(Wj)
        eS += shift(e_d, lens, -sh) @ a64(Wj)
    eS = (k * cout + 1) * U * aS + eS
    return masked(S, aS, eS, x, _slope(slope, mutant), None, ex, None, mutant, dt)


def end_dw(x, wav, dwav, k, lens, slope=OUT_SLOPE, ex=None, ewav=None, edwav=None, mutant=None, dt=np.float64):
    """dW[o, ch, j] = sum_t dpre[t, o] l(x)[t + j - h, ch], db[o] = sum_t dpre[t, o] -> (dW (cout, C, k), db, e_dW, e_db)"""
    f = lambda v: np.asarray(v, dtype=dt)
    n, cin, cout = len(x), x.shape[1], np.shape(wav)[1]
    d, e_d = dpre(wav, dwav, ewav, edwav, mutant, dt)
    a, ea = lrelu(f(x), _slope(slope, mutant)), _z(ex, x)
    across = mutant == "tap_across_edge"
    dW, eW = np.zeros((cout, cin, k), dt), np.zeros((cout, cin, k))
    for j in range(k):
        sh = j - (k - 1) // 2
        aa, ee = shift(a64(a), lens, sh), shift(ea, lens, sh)
        dW[:, :, j] = d.T @ shift(a, lens, sh, across)
        eW[:, :, j] = (n + 2) * U * (a64(d).T @ aa) + e_d.T @ aa + a64(d).T @ ee + e_d.T @ ee
    db = np.zeros(cout, dt) if mutant == "missing_bias_gradient" else d.sum(0)
    return dW, db, eW, (n + 2) * U * a64(d).sum(0) + e_d.sum(0)


def end_case(C, cout, k, lens=LENS):
    """(x [N, C], w (cout, C, k), b [cout], dwav [N, cout]) float32 on `lens`: pre-activations of about unit size, tanh away from saturation"""
    rng = np.random.RandomState(9000 + 100 * C + 10 * cout + k)
    f = lambda *shp: rng.standard_normal(shp).astype(np.float32)
    n = sum(lens)
    return f(n, C), f(cout, C, k) / np.float32(np.sqrt(C * k)), np.float32(0.5) * f(cout), f(n, cout)


def given_wav(x, w, b, lens):
    """the waveform the backward launches take as given: the statement's own, rounded to float32"""
    return np.tanh(end_pre(np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(b, np.float64), lens)[0]).astype(np.float32)


def sweep_case(n=1000000, lo=-9.0, hi=9.0):
    """the E_TANH measurement: C = 16, k = 3, the one nonzero weight W[0, 0, 1] = 1.5 and a zero bias, so that pre = 1.5 l(x[t, 0]) is ONE product of
    an exactly representable LeakyReLU value -> (x [n, 16], w (1, 16, 3), b [1], the float64 pre-activation, e_pre = 2 u |pre|: the LeakyReLU product
    for the negative arguments and the weight product)"""
    x = np.zeros((n, 16), np.float32)
    grid = np.linspace(lo, hi, n)
    x[:, 0] = np.where(grid > 0, grid / 1.5, grid / 1.5 / OUT_SLOPE).astype(np.float32)
    x[:, 1:] = np.random.RandomState(5).standard_normal((n, 15)).astype(np.float32)  # against zero weights
    w = np.zeros((1, 16, 3), np.float32)
    w[0, 0, 1] = 1.5
    pre = 1.5 * lrelu(x[:, :1].astype(np.float64), OUT_SLOPE)
    return x, w, np.zeros(1, np.float32), pre, 2 * U * np.abs(pre)


def generator_bwd(R, sd, cfg, mel, lens, fw, dout, edout):
    """hfgt_ref.generator_bwd with the bound of `dout` (the end's input gradient) carried in: dict grads, e_grads, unsure"""
    nk = len(cfg["resblock_kernel_sizes"])
    rates = [1]
    for s in cfg["upsample_scales"]:
        rates.append(rates[-1] * s)
    g, eg, grads, e_grads, unsure = dout, edout, {}, {}, 0.0
    for i in range(len(cfg["upsample_scales"]) - 1, -1, -1):
        c, ec = (fw["c0"], fw["e_c0"]) if i == 0 else (fw["stages"][i - 1]["out"], fw["stages"][i - 1]["e_out"])
        r = R.stage_bwd(c, fw["stages"][i], R.stage_weights(sd, cfg, i), cfg, i, [n * rates[i] for n in lens], g, R.SLOPE, ec, eg)
        names = ["upsamples.%d.1.weight" % i, "upsamples.%d.1.bias" % i]
        for j in range(nk):
            for d in range(len(cfg["resblock_dilations"][j])):
                p = "blocks.%d." % (i * nk + j)
                names += [p + "convs1.%d.1.weight" % d, p + "convs1.%d.1.bias" % d, p + "convs2.%d.1.weight" % d, p + "convs2.%d.1.bias" % d]
        grads.update(zip(names, r["grads"]))
        e_grads.update(zip(names, r["e_grads"]))
        g, eg, unsure = r["dc"], r["e_dc"], max(unsure, r["unsure"])
    dw, db, e_dw, e_db = R.conv_dw(mel, g, cfg["kernel_size"], 1, lens, R.SLOPE, act=False, eg=eg)
    grads["input_conv.weight"], grads["input_conv.bias"], e_grads["input_conv.weight"], e_grads["input_conv.bias"] = dw, db, e_dw, e_db
    return dict(grads=grads, e_grads=e_grads, unsure=unsure)


def module_statement(R, sd, wo, bo, cfg, mel, lens, dwav, e_tanh=None):
    """the whole generator with its output end, forward and backward from the waveform's gradient dwav [rows x hop, cout], on plain float64 weights (sd:
    input_conv and the stages; wo, bo: output_conv) -> dict wav, e_wav, grads / e_grads by state-dict name (output_conv.1.* included), unsure"""
    hop = int(np.prod(cfg["upsample_scales"]))
    ln = [n * hop for n in lens]
    fw = R.generator_fwd(sd, cfg, mel, lens)
    wav, e_wav = end_fwd(fw["out"], wo, bo, ln, ex=fw["e_out"], e_tanh=e_tanh)
    dx, e_dx, unsure = end_dx(fw["out"], wo, wav, dwav, ln, ex=fw["e_out"], ewav=e_wav)
    dW, db, e_dW, e_db = end_dw(fw["out"], wav, dwav, wo.shape[2], ln, ex=fw["e_out"], ewav=e_wav)
    bw = generator_bwd(R, sd, cfg, mel, lens, fw, dx, e_dx)
    bw["grads"].update({"output_conv.1.weight": dW, "output_conv.1.bias": db})
    bw["e_grads"].update({"output_conv.1.weight": e_dW, "output_conv.1.bias": e_db})
    return dict(wav=wav, e_wav=e_wav, grads=bw["grads"], e_grads=bw["e_grads"], unsure=max(unsure, bw["unsure"]))
