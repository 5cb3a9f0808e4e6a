"""Float64 numpy statement of the multi-resolution STFT loss and of its gradient (include/fcl_hip.h "Multi-resolution STFT loss"): no
package code, and no torch but in torch_statement at the end (torch.stft + autograd: the second statement the first is pinned to).  The inputs of tests/test_gpu_stft_loss.py are built here (CASES, lengths, signals), with the bounds the device results are
held to and the mutants those bounds have to reject, so that tests/test_stft_loss_cpu.py can check all of that without a GPU.

Per resolution (n_fft N, hop, win_length): utterance u has L samples of x (generated) and y (target) and T = L // hop + 1 frames; frame t reads the
padded positions t hop + n - N / 2, n < N, reflected once at either end (L >= N / 2 + 1); the window is the periodic Hann of win_length zero-padded
centred to N; X = rfft(frame w); p = re^2 + im^2, m = sqrt(max(p, 1e-7)) for x and y.  Over a set of frames (one utterance, or the batch):
A = sum (m_y - m_x)^2, B = sum m_y^2, C = sum |log m_y - log m_x|, n = frames (N / 2 + 1); sc = sqrt(A / B), mag = C / n.  "batch": one A, B, C, n
over all frames; "utterance": the means of the per-utterance sc, mag.  The gradient with respect to x for upstream g_sc, g_mag:
dm = c0 (m_y - m_x) - c1 sign(log m_y - log m_x) / m_x with c0 = -g_sc / sqrt(A B), c1 = g_mag / n (under "utterance" the utterance's own, divided
by the number of utterances); G = (dm / m_x) X where p_x > 1e-7, else 0; the frame gradient is w_n Re sum_k G_k e^{+2 pi i k n / N} with each
one-sided bin counted once; d / dx_j is its sum over every (frame, n) whose reflected position is j."""
import numpy as np

import features_ref as F
import griffinlim_ref as R

U = R.U24
CLAMP = 1e-7
DEFAULT_RESOLUTIONS = [(1024, 120, 600), (2048, 240, 1200), (512, 50, 240)]  # Parallel WaveGAN's

# (n_fft, hop, win_length) -> the lengths of its three utterances: the minimum N / 2 + 1 (both mirrors overlap), lengths hop does not divide, frame
# counts that are no multiple of the frames per workgroup (4 / 2 / 1), so that an utterance boundary falls inside a workgroup
CASES = {(512, 50, 240): [257, 700, 1203], (1024, 120, 600): [513, 1300, 2050], (2048, 240, 1200): [1025, 2100, 3333],
         (1024, 256, 1024): [513, 1000, 1537]}
SILENT_CASE = (512, 50, 240)  # the extra case: its middle utterance has x = 0
MODULE_B, MODULE_T = 2, 2100  # the [B, T] input of the module test on the default resolutions
UPSTREAM = (1.0, 1.0)  # g_sc, g_mag of the kernel tests
# per utterance (gain, echo): x = gain y + echo (y delayed by one sample).  |gain + echo e^{-i w}| stays on one side of 1, so log m_y - log m_x keeps
# its sign inside an utterance and differs between them; the echo makes m_x / m_y depend on the bin.  The gains lie far from 1 because the condition
# on the sign (conditions() below) asks |m_y - m_x| of EVERY bin to exceed the frame's magnitude bound, and frame 0 of any utterance is symmetric
# about its centre (the reflection), so its bins are real and small ones are common.
SHAPES = [(0.25, 0.08), (4.0, 0.6), (0.35, -0.05)]
# per utterance the seed, among the first 80 (40 for the default-resolution inputs), whose signal meets conditions() in 100 % of the bins and has the
# smallest gradient bound relative to the gradient's norm -- both read off the float64 statement alone; test_stft_loss_cpu.py asserts the former
# and prints the latter.  The bound puts a frame's whole transform error on its most sensitive bin (the log term's 1 / m_x^2), so it is only as
# tight as the smallest bin of the signal allows.
SEEDS = {(512, 50, 240): (50, 48, 36), (1024, 120, 600): (37, 47, 45), (2048, 240, 1200): (61, 13, 46), (1024, 256, 1024): (22, 30, 78)}
MODULE_SEEDS, RAGGED_SEEDS, RAGGED_LENS = (16, 33), (14, 33, 7), (1025, 1900, 1431)


# ---- the statement ---------------------------------------------------------------------------------------------------------------------------
def window(case):
    return R.hann_window(case[2], case[0])


def frame_index(L, n_fft, hop):
    """[T, n_fft] int: the sample of x each (frame, n) reads"""
    q = np.arange(F.frames_of(L, hop))[:, None] * hop + np.arange(n_fft)[None, :] - n_fft // 2
    q = np.where(q < 0, -q, q)
    return np.where(q >= L, 2 * (L - 1) - q, q)


def spectrum(x, w, hop):
    x = np.asarray(x, dtype=np.float64)
    assert len(x) >= len(w) // 2 + 1
    return np.fft.rfft(x[frame_index(len(x), len(w), hop)] * w, axis=1)


def magnitudes(X):
    return np.sqrt(np.maximum(X.real ** 2 + X.imag ** 2, CLAMP))


def frame_sums(x, y, w, hop):
    """[T, 3]: per frame (sum (m_y - m_x)^2, sum m_y^2, sum |log m_y - log m_x|)"""
    mx, my = magnitudes(spectrum(x, w, hop)), magnitudes(spectrum(y, w, hop))
    return np.stack([((my - mx) ** 2).sum(1), (my ** 2).sum(1), np.abs(np.log(my) - np.log(mx)).sum(1)], axis=1)


def utt_sums(xs, ys, w, hop):
    """[n_utt, 3] and n [n_utt] = frames x bins"""
    s = np.stack([frame_sums(x, y, w, hop).sum(0) for x, y in zip(xs, ys)])
    return s, np.array([F.frames_of(len(x), hop) * (len(w) // 2 + 1) for x in xs], dtype=np.float64)


def figures(s, n, reduction):
    """(sc, mag) of one resolution from the per-utterance sums"""
    if reduction == "batch":
        return np.sqrt(s[:, 0].sum() / s[:, 1].sum()), s[:, 2].sum() / n.sum()
    return np.sqrt(s[:, 0] / s[:, 1]).mean(), (s[:, 2] / n).mean()


def loss(xs, ys, resolutions, reduction):
    """(sc, mag): the means over the resolutions"""
    per = [figures(*utt_sums(xs, ys, window(c), c[1]), reduction) for c in resolutions]
    return float(np.mean([p[0] for p in per])), float(np.mean([p[1] for p in per]))


def coefficients(s, n, g_sc, g_mag, reduction, n_as_frames=None, utt_ab=False):
    """[n_utt, 2]: per utterance (c0, c1) = (-g_sc / sqrt(A B), g_mag / n) with the reduction folded in.  Mutants: n_as_frames (the bins per frame:
    n taken as frames), utt_ab (the utterance's own A, B under "batch")."""
    n = n / n_as_frames if n_as_frames else n
    k = len(n)
    if reduction == "batch":
        ab = s[:, 0] * s[:, 1] if utt_ab else np.full(k, s[:, 0].sum() * s[:, 1].sum())
        return np.stack([-g_sc / np.sqrt(ab), np.full(k, g_mag / n.sum())], axis=1)
    return np.stack([-g_sc / np.sqrt(s[:, 0] * s[:, 1]) / k, g_mag / n / k], axis=1)


def bin_gradient(X, Y, c0, c1, through_clamp=False):
    """G [T, bins] complex"""
    px = X.real ** 2 + X.imag ** 2
    mx, my = magnitudes(X), magnitudes(Y)
    dm = c0 * (my - mx) - c1 * np.sign(np.log(my) - np.log(mx)) / mx
    G = dm / mx * X
    return G if through_clamp else np.where(px > CLAMP, G, 0.0)


def utt_gradient(x, y, w, hop, c0, c1, double_interior=False, no_reflection=False, no_window=False, through_clamp=False, w_bwd=None):
    """d / dx of c0-, c1-weighted sums of one utterance; the keyword flags are the mutants"""
    n_fft, L = len(w), len(x)
    G = bin_gradient(spectrum(x, w, hop), spectrum(y, w, hop), c0, c1, through_clamp)
    k, n = np.arange(n_fft // 2 + 1), np.arange(n_fft)
    count = np.ones(len(k)) if not double_interior else np.where((k == 0) | (k == n_fft // 2), 1.0, 2.0)
    gf = (G * count) @ np.exp(2j * np.pi * np.outer(k, n) / n_fft)  # each one-sided bin once
    gf = gf.real * (1.0 if no_window else (w if w_bwd is None else w_bwd))
    gx = np.zeros(L)
    if no_reflection:  # only the positions that lie inside the utterance
        q = np.arange(gf.shape[0])[:, None] * hop + n[None, :] - n_fft // 2
        ok = (q >= 0) & (q < L)
        np.add.at(gx, q[ok], gf[ok])
    else:
        np.add.at(gx, frame_index(L, n_fft, hop), gf)
    return gx


def gradient(xs, ys, case, g_sc, g_mag, reduction, coef=None, **mutant):
    """per utterance d (g_sc sc + g_mag mag) / dx of one resolution"""
    w = window(case)
    if coef is None:
        coef = coefficients(*utt_sums(xs, ys, w, case[1]), g_sc, g_mag, reduction)
    return [utt_gradient(x, y, w, case[1], c[0], c[1], **mutant) for x, y, c in zip(xs, ys, coef)]


def total_gradient(xs, ys, resolutions, g_sc, g_mag, reduction):
    """per utterance, over the resolutions (each takes g / R)"""
    R_ = len(resolutions)
    per = [gradient(xs, ys, c, g_sc / R_, g_mag / R_, reduction) for c in resolutions]
    return [sum(p[u] for p in per) for u in range(len(xs))]


# ---- bounds: derived, not measured ------------------------------------------------------------------------------------------------------------
SUM_U = 16  # roundings on the longest path of a frame's float32 sum: <= 5 FMAs per thread, a tree of <= 8 levels, the store


def all_clamped(x, w, hop):
    """every bin of x has p <= 1e-7 / 4 (digital silence, or next to it): m_x sits at the clamp in float32 as in float64 and G is exactly 0"""
    X = spectrum(x, w, hop)
    return bool((X.real ** 2 + X.imag ** 2 <= CLAMP / 4).all())


def mag_delta(X, n_fft):
    """per frame: ||m_gpu - m||_2 <= fft_bound ||X||_2 + 4 U ||m||_2  (features_ref.magnitude_bound: |.| and the clamp are 1-Lipschitz; 4 U for p and
    its root, which a bin at the clamp carries too)"""
    return R.fft_bound(n_fft) * np.linalg.norm(X, axis=1) + 4 * U * np.linalg.norm(magnitudes(X), axis=1)


def frame_sum_bounds(x, y, w, hop):
    """[T, 3]: |dA| <= 2 sqrt(A) d + d^2 + SUM_U U A with d = dx + dy (the error of m_y - m_x in the 2-norm); |dB| likewise with dy; |dC| <=
    (dx ||1 / m_x||_2 + dy ||1 / m_y||_2) / (1 - r) + sum_k 4 U max(1, |log m|) (logf, twice) + (SUM_U + 2) U C, r = max(dx / min m_x, dy / min m_y)
    (|log(1 + e)| <= |e| / (1 - |e|), Cauchy-Schwarz over the bins)"""
    n_fft = len(w)
    X, Y = spectrum(x, w, hop), spectrum(y, w, hop)
    mx, my = magnitudes(X), magnitudes(Y)
    dx, dy = mag_delta(X, n_fft), mag_delta(Y, n_fft)
    s = frame_sums(x, y, w, hop)
    d = dx + dy
    r = np.maximum(dx / mx.min(1), dy / my.min(1))
    assert (r < 0.5).all()
    bc = (dx * np.linalg.norm(1 / mx, axis=1) + dy * np.linalg.norm(1 / my, axis=1)) / (1 - r)
    bc += 4 * U * (np.maximum(1, np.abs(np.log(mx))) + np.maximum(1, np.abs(np.log(my)))).sum(1) + (SUM_U + 2) * U * s[:, 2]
    return np.stack([2 * np.sqrt(s[:, 0]) * d + d * d + SUM_U * U * s[:, 0], 2 * np.sqrt(s[:, 1]) * dy + dy * dy + SUM_U * U * s[:, 1], bc], axis=1)


def figure_bounds(s, b, n, reduction):
    """(|d sc|, |d mag|) of one resolution, first order: sc = sqrt(A / B): sc (dA / A + dB / B) / 2; mag = C / n; 4 U for the float32 result"""
    if reduction == "batch":
        s, b, n = s.sum(0)[None], b.sum(0)[None], n.sum()[None]
    sc = np.sqrt(s[:, 0] / s[:, 1])
    return float((sc * (0.5 * (b[:, 0] / s[:, 0] + b[:, 1] / s[:, 1]) + 4 * U)).mean()), float((b[:, 2] / n + 4 * U * s[:, 2] / n).mean())


def gradient_bounds(xs, ys, case, coef, sum_rel):
    """eps_u with ||g_gpu - g||_2 <= eps_u, per utterance, to first order.  sum_rel [n_utt]: the relative bound of the utterance's A B product
    (dA / A + dB / B over the set its c0 comes from), so |d c0| <= |c0| (sum_rel / 2 + 2 U).  Per frame, G_k = s_k X_k with
    s = c0 (m_y / m_x - 1) - c1 sign / m_x^2:
      |dG| <= |ds| m_x + |s| |dX|,  ds = (ds / dm_x) dm_x + (ds / dm_y) dm_y + (m_y / m_x - 1) dc0 + rounding
      (ds / dm_x) m_x = -(c0 m_y / m_x - 2 c1 sign / m_x^2) =: -a,  (ds / dm_y) m_x = c0
      ||dG||_2 <= max|a| dx + |c0| dy + max|s| fft_bound ||X||_2 + |dc0| sqrt(A_t) + 8 U (|c0| (||m_x|| + ||m_y||) + |c1| ||1 / m_x||)
    The frame gradient is w N irfft(Yh) with ||N irfft(Yh)||_2 <= sqrt(N) ||G||_2 (Parseval, w <= 1), the inverse transform adds fft_bound of that:
      e_t = sqrt(N) (||dG||_2 + (fft_bound + 2 U) ||G||_2)
    Sample j sums the c_j (frame, n) pairs that read it, so ||d gx||_2 <= sqrt(c_max sum_t e_t^2) (Cauchy-Schwarz per sample) and the float32 sum
    itself adds c_max U sqrt(c_max sum_t ||gf_t||^2).  An utterance whose bins are all_clamped has G = 0 in float32 as in float64: eps = 0."""
    n_fft, hop, _ = case
    w, fb = window(case), R.fft_bound(n_fft)
    out = []
    for x, y, (c0, c1), rel in zip(xs, ys, coef, sum_rel):
        if all_clamped(x, w, hop):
            out.append(0.0)
            continue
        X, Y = spectrum(x, w, hop), spectrum(y, w, hop)
        mx, my = magnitudes(X), magnitudes(Y)
        dx, dy = mag_delta(X, n_fft), mag_delta(Y, n_fft)
        sg = np.sign(np.log(my) - np.log(mx))
        s = c0 * (my / mx - 1) - c1 * sg / mx ** 2
        a = c0 * my / mx - 2 * c1 * sg / mx ** 2
        dc0 = abs(c0) * (0.5 * rel + 2 * U)
        nX = np.linalg.norm(X, axis=1)
        dG = (np.abs(a).max(1) * dx + abs(c0) * dy + np.abs(s).max(1) * fb * nX + dc0 * np.linalg.norm(my - mx, axis=1)
              + 8 * U * (abs(c0) * (np.linalg.norm(mx, axis=1) + np.linalg.norm(my, axis=1)) + abs(c1) * np.linalg.norm(1 / mx, axis=1)))
        nG = np.linalg.norm(s * mx, axis=1)
        e = np.sqrt(n_fft) * (dG + (fb + 2 * U) * nG)
        c_max = np.bincount(frame_index(len(x), n_fft, hop).ravel()).max()
        out.append(float(np.sqrt(c_max * (e ** 2).sum()) + c_max * U * np.sqrt(c_max * n_fft * (nG ** 2).sum())))
    return np.array(out)


def kernel_reference(case, xs, ys, reduction="utterance", upstream=UPSTREAM):
    """everything one kernel test compares against, and its bounds"""
    w, hop = window(case), case[1]
    fs = [frame_sums(x, y, w, hop) for x, y in zip(xs, ys)]
    fb = [frame_sum_bounds(x, y, w, hop) for x, y in zip(xs, ys)]
    s, b = np.stack([f.sum(0) for f in fs]), np.stack([f.sum(0) for f in fb])
    n = np.array([len(f) * (case[0] // 2 + 1) for f in fs], dtype=np.float64)
    coef = coefficients(s, n, upstream[0], upstream[1], reduction)
    rel = b[:, 0] / s[:, 0] + b[:, 1] / s[:, 1] if reduction == "utterance" else np.full(len(xs), b[:, 0].sum() / s[:, 0].sum() + b[:, 1].sum() / s[:, 1].sum())
    return dict(frame_sums=np.concatenate(fs), frame_bounds=np.concatenate(fb), utt_sums=s, utt_bounds=b, n=n, coef=coef,
                grad=gradient(xs, ys, case, upstream[0], upstream[1], reduction, coef=coef), grad_bounds=gradient_bounds(xs, ys, case, coef, rel))


def module_reference(xs, ys, resolutions, reduction, g_sc=1.0, g_mag=1.0):
    """(sc, mag), per-utterance gradient of g_sc sc + g_mag mag, and the bounds combined over the resolutions: the mean of the figures' bounds; the
    sum of the gradients' bounds at g / R plus 2 U per float32 addition of a resolution's share"""
    Rn = len(resolutions)
    refs = [kernel_reference(c, xs, ys, reduction, (g_sc / Rn, g_mag / Rn)) for c in resolutions]
    fig = [figures(r["utt_sums"], r["n"], reduction) for r in refs]
    fbd = [figure_bounds(r["utt_sums"], r["utt_bounds"], r["n"], reduction) for r in refs]
    grad = [sum(r["grad"][u] for r in refs) for u in range(len(xs))]
    gb = sum(r["grad_bounds"] for r in refs) + 2 * U * Rn * np.array([sum(np.linalg.norm(r["grad"][u]) for r in refs) for u in range(len(xs))])
    return dict(sc=float(np.mean([f[0] for f in fig])), mag=float(np.mean([f[1] for f in fig])), sc_bound=float(np.mean([f[0] for f in fbd])) + 4 * U,
                mag_bound=float(np.mean([f[1] for f in fbd])) + 4 * U, grad=grad, grad_bounds=gb)


# ---- conditions on the inputs -------------------------------------------------------------------------------------------------------------------
def conditions(case, xs, ys):
    """the share of bins (1.0 is required) that meet: p >= 4e-7 for x and y; m - delta above the clamp's sqrt(1e-7) and delta < m / 2 (the clamp
    cannot flip within the magnitude bound); |m_y - m_x| > delta_x + delta_y (nor can the sign).  Utterances whose x is all_clamped are left out."""
    w, hop, n_fft = window(case), case[1], case[0]
    ok = tot = 0
    for x, y in zip(xs, ys):
        if all_clamped(x, w, hop):
            continue
        X, Y = spectrum(x, w, hop), spectrum(y, w, hop)
        mx, my = magnitudes(X), magnitudes(Y)
        dx, dy = mag_delta(X, n_fft)[:, None], mag_delta(Y, n_fft)[:, None]
        good = (np.abs(X) ** 2 >= 4e-7) & (np.abs(Y) ** 2 >= 4e-7) & (mx - dx > np.sqrt(CLAMP)) & (my - dy > np.sqrt(CLAMP)) & (2 * dx < mx) & (2 * dy < my)
        good &= np.abs(my - mx) > dx + dy
        ok, tot = ok + int(good.sum()), tot + good.size
    return ok / tot


# ---- the inputs of tests/test_gpu_stft_loss.py ------------------------------------------------------------------------------------------------------
def pair(seed, L, shape, n_fft):
    """(x, y) rounded to float32.  y: a speech-like burst -- partials over noise (griffinlim_ref.signal) under an envelope that opens over the first
    and closes over the last n_fft / 2 samples (floor 0.01), a click at the first and at the last sample, and a small offset at DC and at the Nyquist
    frequency.  The frames at either end are symmetric about a reflection point, so their bins are real and small ones would be common; there the
    click, which sits on the point itself, gives every bin the same magnitude and the envelope keeps the noise below it.  The offsets do the same
    for the two real bins of every other frame.  x = gain y + echo y[. - 1]."""
    i = np.arange(L)
    env = np.maximum(0.01, np.minimum(1.0, np.minimum(i, L - 1 - i) / (n_fft / 2.0)) ** 2)
    y = R.signal(seed, L) * env + 0.05 + 0.05 * (-1.0) ** i
    y[0] += 0.9
    y[L - 1] += 0.9
    y = y.astype(np.float32).astype(np.float64)
    gain, echo = shape
    x = gain * y + echo * np.concatenate([[y[0]], y[:-1]])
    return x.astype(np.float32), y.astype(np.float32)


def signals(case, silent=False):
    """(xs, ys) of a case: three utterances; silent: the middle one has x = 0"""
    ps = [pair(SEEDS[case][j], L, SHAPES[j], case[0]) for j, L in enumerate(CASES[case])]
    xs, ys = [p[0] for p in ps], [p[1] for p in ps]
    if silent:
        xs[1] = np.zeros_like(xs[1])
    return xs, ys


def module_signals():
    """equal-length clips for the [B, T] form"""
    ps = [pair(MODULE_SEEDS[j], MODULE_T, SHAPES[j + 1], 2048) for j in range(MODULE_B)]
    return [p[0] for p in ps], [p[1] for p in ps]


def ragged_signals():
    """a ragged batch for the default resolutions: every utterance at least 2048 / 2 + 1 samples"""
    ps = [pair(RAGGED_SEEDS[j], L, SHAPES[j], 2048) for j, L in enumerate(RAGGED_LENS)]
    return [p[0] for p in ps], [p[1] for p in ps]


def quiet_signals(case):
    """signals(case) with the middle x scaled until every bin of it lies below the clamp (p_x < 1e-7 / 4) without being zero: the gradient of that
    utterance is exactly zero, which the mutant that passes a gradient through the clamp does not give"""
    xs, ys = signals(case)
    xs[1] = (xs[1].astype(np.float64) * 1e-7).astype(np.float32)
    return xs, ys


# ---- mutants of the window ------------------------------------------------------------------------------------------------------------------------
def left_aligned_window(case):
    out = np.zeros(case[0])
    out[: case[2]] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(case[2]) / case[2])
    return out


def symmetric_window(case):
    return F.symmetric_hann(case[2], case[0])


# ---- the same loss as torch.stft + autograd ----------------------------------------------------------------------------------------------------------
def torch_statement(xs, ys, resolutions, reduction, g_sc=1.0, g_mag=1.0, dtype=None, detail=False):
    """(sc, mag, per-utterance gradient of g_sc sc + g_mag mag) on the CPU in `dtype` (float64 by default); detail: also, per resolution, the
    per-frame sums [frames, 3] as numpy"""
    import torch

    dtype = torch.float64 if dtype is None else dtype
    tx = [torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True) for x in xs]
    ty = [torch.tensor(np.asarray(y), dtype=dtype) for y in ys]
    scs, mags, frames = [], [], []
    for n_fft, hop, wl in resolutions:
        win = torch.hann_window(wl, dtype=dtype)
        per = []
        for x, y in zip(tx, ty):
            m = []
            for v in (x, y):
                S = torch.stft(v, n_fft, hop, wl, win, center=True, pad_mode="reflect", return_complex=True).transpose(0, 1)
                m.append(torch.sqrt(torch.clamp(S.real ** 2 + S.imag ** 2, min=CLAMP)))
            per.append(torch.stack([((m[1] - m[0]) ** 2).sum(1), (m[1] ** 2).sum(1), (torch.log(m[1]) - torch.log(m[0])).abs().sum(1)], dim=1))
        frames.append(np.concatenate([p.detach().numpy() for p in per]))
        s = torch.stack([p.sum(0) for p in per])
        n = torch.tensor([p.shape[0] * (n_fft // 2 + 1) for p in per], dtype=dtype)
        if reduction == "batch":
            scs.append(torch.sqrt(s[:, 0].sum() / s[:, 1].sum()))
            mags.append(s[:, 2].sum() / n.sum())
        else:
            scs.append(torch.sqrt(s[:, 0] / s[:, 1]).mean())
            mags.append((s[:, 2] / n).mean())
    sc, mag = torch.stack(scs).mean(), torch.stack(mags).mean()
    (g_sc * sc + g_mag * mag).backward()
    out = (float(sc.detach()), float(mag.detach()), [x.grad.numpy().astype(np.float64) for x in tx])
    return out + (frames,) if detail else out
