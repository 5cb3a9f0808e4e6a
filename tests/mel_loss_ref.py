"""Float64 numpy statement of the mel-spectrogram L1 loss and of its gradient (include/fcl_hip.h "Mel-spectrogram loss"): no package
code, and no torch but in torch_statement at the end (torch.stft + matmul + log10 + autograd: the second statement the first is pinned to).  The
inputs of tests/test_gpu_mel_loss.py are built here (CASES, signals, mel matrices), with the bounds the device results are held to and the mutants
those bounds have to reject, so that tests/test_mel_loss_cpu.py can check all of that without a GPU.

Per resolution (n_fft N, hop, win_length, mel matrix B [n_mels, N / 2 + 1]): utterances, frames, reflection, window and X = rfft(frame w) are those of
stft_loss_ref.py.  p = re^2 + im^2, m = sqrt(max(p, 1e-10)) for x and y; M_c = max(sum_k m_k B[c, k], 1e-10); l_c = log10 M_c;
D = sum over (frame, channel) of |l_x - l_y|; n = frames n_mels.  "batch": D / n over all frames; "utterance": the mean of the per-utterance D / n.
The gradient with respect to x for upstream g: dl_c = kappa sign(l_x,c - l_y,c) / M_x,c where the sum exceeds 1e-10 (else 0), kappa = g / (ln 10 n)
with the reduction folded in; dm_k = sum_c B[c, k] dl_c; G_k = (dm_k / m_x,k) X_k where p_x > 1e-10 (else 0); from G on as the STFT loss: the frame
gradient is w_n Re sum_k G_k e^{+2 pi i k n / N} with each one-sided bin counted once, d / dx_j its sum over every (frame, n) whose reflected
position is j."""
import numpy as np

import features_ref as F
import griffinlim_ref as R
import stft_loss_ref as S

U = R.U24
FLOOR = 1e-10
LN10 = float(np.log(10.0))
MEL = dict(fs=22050, fmin=80.0, fmax=7600.0)
DEFAULT_RESOLUTIONS = [(1024, 256, 1024, 80)]  # features.DEFAULTS
THREE_RESOLUTIONS = [(1024, 256, 1024, 80), (2048, 240, 1200, 80), (512, 50, 240, 80)]

# (n_fft, hop, win_length, n_mels | "hand"): the geometries, lengths and (gain, echo) shapes of stft_loss_ref.CASES -- the minimum N / 2 + 1, a length
# hop does not divide, a frame count that is no multiple of the frames per workgroup -- at 80 mels; 13 mels (FPW n_mels is no multiple of the block,
# wide bands); 256 mels at n_fft 512 (the LDS limit; triangles narrower than a bin: all-zero rows); and the hand-made matrix of hand_basis().
CASES = [(512, 50, 240, 80), (1024, 120, 600, 80), (2048, 240, 1200, 80), (1024, 256, 1024, 13), (512, 50, 240, 256), (512, 50, 240, "hand")]
SILENT_CASE = (512, 50, 240, 80)
MODULE_B, MODULE_T = S.MODULE_B, S.MODULE_T
# per utterance the seed, among the first 80 (40 for the module's inputs, which have to serve three resolutions at once), whose signal meets
# conditions() in 100 % of the cells and bins and has the smallest gradient bound relative to the gradient's norm (the module's: summed over
# THREE_RESOLUTIONS, and over z and 0.9 z for the clips the graph test scales) -- both read off the float64 statement alone; 64 - 80 of the 80
# (37 - 39 of the 40) seeds meet the conditions.  test_mel_loss_cpu.py asserts the former and prints the latter.
SEEDS = {(512, 50, 240, 80): (50, 66, 17), (1024, 120, 600, 80): (74, 4, 62), (2048, 240, 1200, 80): (48, 60, 63), (1024, 256, 1024, 13): (45, 73, 78),
         (512, 50, 240, 256): (50, 66, 36), (512, 50, 240, "hand"): (14, 44, 48)}
MODULE_SEEDS, RAGGED_SEEDS, RAGGED_LENS = (0, 38), (38, 33, 9), S.RAGGED_LENS


# ---- mel matrices -------------------------------------------------------------------------------------------------------------------------------
def hand_basis(bins=257):
    """a hand-made [6, bins] matrix of contiguous bands: row 2 all zero; bins 40 .. 49 covered by the three rows 0, 3, 5 (and 44 .. 49 by row 4 too),
    which are no contiguous run of channels; the bands' first bins (10, 150, -, 30, 44, 5) are not in ascending order"""
    B = np.zeros((6, bins))
    k = np.arange(bins)
    for c, (a, b) in {0: (10, 60), 1: (150, bins), 3: (30, 50), 4: (44, 120), 5: (5, 90)}.items():
        B[c, a:b] = (0.002 + 0.02 * np.sin(np.pi * (k[a:b] - a + 0.5) / (b - a)) ** 2) * (1.0 + 0.25 * c)
    return B


def filterbank(case):
    n_fft, n_mels = case[0], case[3]
    return hand_basis(n_fft // 2 + 1) if n_mels == "hand" else R.mel_filterbank(MEL["fs"], n_fft, n_mels, MEL["fmin"], MEL["fmax"])


def banded32(B):
    """B with its weights rounded to float32 (what the device holds), as float64"""
    return np.asarray(B, dtype=np.float32).astype(np.float64)


# ---- the statement ---------------------------------------------------------------------------------------------------------------------------
def window(case):
    return S.window(case[:3])


def magnitudes(X, floor=FLOOR):
    return np.sqrt(np.maximum(X.real ** 2 + X.imag ** 2, floor))


def mels(X, B, floor=FLOOR):
    """(sum before the floor, M) [T, n_mels]"""
    A = magnitudes(X, floor) @ np.asarray(B, dtype=np.float64).T
    return A, np.maximum(A, FLOOR)


def frame_sums(x, y, w, hop, B, log=np.log10, floor=FLOOR):
    """[T]: per frame sum_c |l_x - l_y|"""
    return np.abs(log(mels(S.spectrum(x, w, hop), B, floor)[1]) - log(mels(S.spectrum(y, w, hop), B, floor)[1])).sum(1)


def utt_sums(xs, ys, w, hop, B, **kw):
    """D [n_utt] and n [n_utt] = frames x n_mels"""
    d = np.array([frame_sums(x, y, w, hop, B, **kw).sum() for x, y in zip(xs, ys)])
    return d, np.array([F.frames_of(len(x), hop) * len(B) for x in xs], dtype=np.float64)


def figure(d, n, reduction):
    return float(d.sum() / n.sum()) if reduction == "batch" else float((d / n).mean())


def loss(xs, ys, cases, reduction, bases=None):
    """the mean over the resolutions"""
    bases = [filterbank(c) for c in cases] if bases is None else bases
    return float(np.mean([figure(*utt_sums(xs, ys, window(c), c[1], B), reduction) for c, B in zip(cases, bases)]))


def coefficients(n, g, reduction, n_as_frames=None):
    """kappa [n_utt] = g / (ln 10 n) with the reduction folded in.  Mutant n_as_frames (= n_mels): n taken as frames without n_mels."""
    n = n / n_as_frames if n_as_frames else n
    return np.full(len(n), g / (LN10 * n.sum())) if reduction == "batch" else g / (LN10 * n * len(n))


def bin_gradient(X, Y, B, kappa, natural_log=False, through_floor=False, first_channel_only=False):
    """G [T, bins] complex; the keyword flags are the mutants"""
    B = np.asarray(B, dtype=np.float64)
    px, mx = X.real ** 2 + X.imag ** 2, magnitudes(X)
    (ax, Mx), (_, My) = mels(X, B), mels(Y, B)
    dl = np.where(ax > FLOOR, kappa * np.sign(np.log10(Mx) - np.log10(My)) / Mx, 0.0) * (LN10 if natural_log else 1.0)
    Bb = B
    if first_channel_only:  # the back-projection keeps the first channel that covers a bin
        first = np.argmax(B != 0, axis=0)
        Bb = np.where(np.arange(len(B))[:, None] == first[None, :], B, 0.0)
    G = (dl @ Bb) / mx * X
    return G if through_floor else np.where(px > FLOOR, G, 0.0)


def frames_to_samples(G, L, w, hop, double_interior=False, no_reflection=False, no_window=False, w_bwd=None):
    """G [T, bins] -> d / dx [L]: each one-sided bin once, times the window, the adjoint of the reflected framing"""
    n_fft = len(w)
    k, n = np.arange(n_fft // 2 + 1), np.arange(n_fft)
    count = np.ones(len(k)) if not double_interior else np.where((k == 0) | (k == n_fft // 2), 1.0, 2.0)
    gf = ((G * count) @ np.exp(2j * np.pi * np.outer(k, n) / n_fft)).real * (1.0 if no_window else (w if w_bwd is None else w_bwd))
    gx = np.zeros(L)
    if no_reflection:
        q = np.arange(gf.shape[0])[:, None] * hop + n[None, :] - n_fft // 2
        ok = (q >= 0) & (q < L)
        np.add.at(gx, q[ok], gf[ok])
    else:
        np.add.at(gx, S.frame_index(L, n_fft, hop), gf)
    return gx


def utt_gradient(x, y, w, hop, B, kappa, natural_log=False, through_floor=False, first_channel_only=False, **framing):
    G = bin_gradient(S.spectrum(x, w, hop), S.spectrum(y, w, hop), B, kappa, natural_log, through_floor, first_channel_only)
    return frames_to_samples(G, len(x), w, hop, **framing)


def gradient(xs, ys, case, g, reduction, B=None, coef=None, **mutant):
    """per utterance d (g loss) / dx of one resolution"""
    w, B = window(case), filterbank(case) if B is None else B
    if coef is None:
        coef = coefficients(utt_sums(xs, ys, w, case[1], B)[1], g, reduction)
    return [utt_gradient(x, y, w, case[1], B, c, **mutant) for x, y, c in zip(xs, ys, coef)]


# ---- bounds: derived, not measured ------------------------------------------------------------------------------------------------------------
SUM_U = S.SUM_U  # roundings on the longest path of a frame's float32 sum: <= 4 additions per thread, a tree of <= 8 levels, the store


def all_floored(x, w, hop):
    """every bin of x has p <= 1e-10 / 4: m_x sits at the floor in float32 as in float64 and G is exactly 0"""
    X = S.spectrum(x, w, hop)
    return bool((X.real ** 2 + X.imag ** 2 <= FLOOR / 4).all())


def band_lengths(B):
    nz = np.asarray(B) != 0
    return np.where(nz.any(1), nz.shape[1] - np.argmax(nz[:, ::-1], axis=1) - np.argmax(nz, axis=1), 0)


def mel_delta(X, B, n_fft):
    """(dM [T, n_mels], M, r): |M_gpu - M| <= ||B_c||_2 d + (band length + 1) U M_c with d = stft_loss_ref.mag_delta, the frame's magnitude error in
    the 2-norm (Cauchy-Schwarz over the band; the FMA chain over the band and the rounding of its weights); r = dM / M.  An all-zero row: 0."""
    B = np.asarray(B, dtype=np.float64)
    _, M = mels(X, B)
    dM = np.linalg.norm(B, axis=1)[None, :] * S.mag_delta(X, n_fft)[:, None] + (band_lengths(B)[None, :] + 1) * U * M
    dM = np.where(B.any(1)[None, :], dM, 0.0)
    return dM, M, dM / M


def log_delta(X, B, n_fft):
    """[T, n_mels]: |l_gpu - l| <= dM / (ln 10 M (1 - r)) + 4 U max(1, |l|) (log10f and the rounding of its result); an all-zero row gives
    log10(1e-10) on either side in either precision: 0"""
    B = np.asarray(B, dtype=np.float64)
    dM, M, r = mel_delta(X, B, n_fft)
    assert (r < 0.5).all()
    return np.where(B.any(1)[None, :], dM / (LN10 * M * (1 - r)) + 4 * U * np.maximum(1.0, np.abs(np.log10(M))), 0.0)


def frame_sum_bounds(x, y, w, hop, B):
    """[T]: |dD_t| <= sum_c (dl_x + dl_y) + (SUM_U + 2) U D_t"""
    n_fft = len(w)
    return (log_delta(S.spectrum(x, w, hop), B, n_fft) + log_delta(S.spectrum(y, w, hop), B, n_fft)).sum(1) + (SUM_U + 2) * U * frame_sums(x, y, w, hop, B)


def figure_bound(d, b, n, reduction):
    """|d loss| of one resolution: dD / n, 4 U for the float32 result"""
    if reduction == "batch":
        return float(b.sum() / n.sum() + 4 * U * d.sum() / n.sum())
    return float((b / n + 4 * U * d / n).mean())


def gradient_bounds(xs, ys, case, B, coef):
    """eps_u with ||g_gpu - g||_2 <= eps_u per utterance, to first order, under conditions().  Per frame, with kappa's float32 rounding (U):
      dl_c = kappa sign / M_c:     |d dl_c| <= |dl_c| (r_c / (1 - r_c) + 4 U)                              (1 / M; kappa, the division, the product)
      dm_k = sum_c B[c, k] dl_c:   |d dm| <= B^T |d dl| + (cover_k + 1) U B^T |dl|                         (the FMA chain over the bin's channels)
      G_k = dm_k X_k / m_k:        ||dG||_2 <= ||d dm||_2 + 2 max_k (|dm_k| / m_k) fft_bound ||X||_2 + 4 U ||dm||_2
                                   (|d (X / m)| <= 2 |dX| / m, the frame's whole transform error on its most sensitive bin)
    then as stft_loss_ref.gradient_bounds: e_t = sqrt(N) (||dG||_2 + (fft_bound + 2 U) ||G||_2) (Parseval, w <= 1, the inverse transform's own error),
    ||d gx||_2 <= sqrt(c_max sum_t e_t^2) + c_max U sqrt(c_max N sum_t ||G_t||^2) (a sample sums the c_j pairs that read it).  An utterance whose
    bins are all_floored has G = 0 in float32 as in float64: eps = 0."""
    n_fft, hop = case[0], case[1]
    w, fb, B = window(case), R.fft_bound(n_fft), np.asarray(B, dtype=np.float64)
    cover = (B != 0).sum(0)
    out = []
    for x, y, kappa in zip(xs, ys, coef):
        if all_floored(x, w, hop):
            out.append(0.0)
            continue
        X, Y = S.spectrum(x, w, hop), S.spectrum(y, w, hop)
        mx = magnitudes(X)
        dM, M, r = mel_delta(X, B, n_fft)
        dl = np.abs(kappa) / M * B.any(1)[None, :]
        ddl = dl * (r / (1 - r) + 4 * U)
        dm = dl @ B  # >= |dm|: the signs taken as equal
        ddm = ddl @ B + (cover[None, :] + 1) * U * dm
        G = np.abs(bin_gradient(X, Y, B, kappa))
        dG = np.linalg.norm(ddm, axis=1) + 2 * (G / mx).max(1) * fb * np.linalg.norm(X, axis=1) + 4 * U * np.linalg.norm(dm, axis=1)
        nG = np.linalg.norm(G, axis=1)
        e = np.sqrt(n_fft) * (dG + (fb + 2 * U) * nG)
        c_max = np.bincount(S.frame_index(len(x), n_fft, hop).ravel()).max()
        out.append(float(np.sqrt(c_max * (e ** 2).sum()) + c_max * U * np.sqrt(c_max * n_fft * (nG ** 2).sum())))
    return np.array(out)


def kernel_reference(case, xs, ys, reduction="utterance", upstream=1.0, B=None):
    """everything one kernel test compares against, and its bounds; the mel matrix is the float32-rounded one the device holds"""
    w, hop = window(case), case[1]
    B = banded32(filterbank(case) if B is None else B)
    fs = [frame_sums(x, y, w, hop, B) for x, y in zip(xs, ys)]
    fb = [frame_sum_bounds(x, y, w, hop, B) for x, y in zip(xs, ys)]
    d, b = np.array([f.sum() for f in fs]), np.array([f.sum() for f in fb])
    n = np.array([len(f) * len(B) for f in fs], dtype=np.float64)
    coef = coefficients(n, upstream, reduction)
    return dict(frame_sums=np.concatenate(fs), frame_bounds=np.concatenate(fb), utt_sums=d, utt_bounds=b, n=n, coef=coef, B=B,
                grad=gradient(xs, ys, case, upstream, reduction, B=B, coef=coef), grad_bounds=gradient_bounds(xs, ys, case, B, coef))


def module_reference(xs, ys, cases, reduction, g=1.0, bases=None):
    """the loss, the per-utterance gradient of g loss and the bounds combined over the resolutions: the mean of the figures' bounds; the sum of the
    gradients' bounds at g / R plus 2 U per float32 addition of a resolution's share"""
    Rn = len(cases)
    refs = [kernel_reference(c, xs, ys, reduction, g / Rn, None if bases is None else bases[i]) for i, c in enumerate(cases)]
    grad = [sum(r["grad"][u] for r in refs) for u in range(len(xs))]
    gb = sum(r["grad_bounds"] for r in refs) + 2 * U * Rn * np.array([sum(np.linalg.norm(r["grad"][u]) for r in refs) for u in range(len(xs))])
    val = float(np.mean([figure(r["utt_sums"], r["n"], reduction) for r in refs]))
    bound = float(np.mean([figure_bound(r["utt_sums"], r["utt_bounds"], r["n"], reduction) for r in refs])) + 4 * U * val
    return dict(loss=val, loss_bound=bound, grad=grad, grad_bounds=gb)


# ---- conditions on the inputs -------------------------------------------------------------------------------------------------------------------
def conditions(case, xs, ys, B=None):
    """the share (1.0 is required) of bins and of (frame, channel) cells that meet, in float64 alone: on every bin that carries weight p >= 4e-10 for
    x and y, m - delta above the floor's sqrt(1e-10) and delta < m / 2 (the magnitude floor cannot flip within the frame's magnitude bound); in
    every cell of a row that is not all zero M - dM > 2e-10 (nor can the mel floor) and |l_x - l_y| > dl_x + dl_y (nor the sign).  Utterances whose x
    is all_floored are left out; the cells of an all-zero row are log10(1e-10) on either side in either precision."""
    w, hop, n_fft = window(case), case[1], case[0]
    B = banded32(filterbank(case) if B is None else B)
    carries, live = B.any(0), B.any(1)
    ok = tot = 0
    for x, y in zip(xs, ys):
        if all_floored(x, w, hop):
            continue
        X, Y = S.spectrum(x, w, hop), S.spectrum(y, w, hop)
        for Z in (X, Y):
            m, d = magnitudes(Z)[:, carries], S.mag_delta(Z, n_fft)[:, None]
            good = (np.abs(Z[:, carries]) ** 2 >= 4 * FLOOR) & (m - d > np.sqrt(FLOOR)) & (2 * d < m)
            ok, tot = ok + int(good.sum()), tot + good.size
        (dMx, Mx, _), (dMy, My, _) = mel_delta(X, B, n_fft), mel_delta(Y, B, n_fft)
        good = (Mx - dMx > 2 * FLOOR) & (My - dMy > 2 * FLOOR) & (np.abs(np.log10(Mx) - np.log10(My)) > log_delta(X, B, n_fft) + log_delta(Y, B, n_fft))
        ok, tot = ok + int(good[:, live].sum()), tot + good[:, live].size
    return ok / tot


# ---- the inputs of tests/test_gpu_mel_loss.py ---------------------------------------------------------------------------------------------------
def signals(case, silent=False):
    """(xs, ys) of a case: stft_loss_ref's three utterances (x = gain y + echo); silent: the middle one has x = 0"""
    ps = [S.pair(SEEDS[case][j], L, S.SHAPES[j], case[0]) for j, L in enumerate(S.CASES[case[:3]])]
    xs, ys = [p[0] for p in ps], [p[1] for p in ps]
    if silent:
        xs[1] = np.zeros_like(xs[1])
    return xs, ys


def lengths(case):
    return S.CASES[case[:3]]


def module_signals():
    """equal-length clips for the [B, T] form"""
    ps = [S.pair(MODULE_SEEDS[j], MODULE_T, S.SHAPES[j + 1], 2048) for j in range(MODULE_B)]
    return [p[0] for p in ps], [p[1] for p in ps]


def ragged_signals():
    """a ragged batch for three resolutions: every utterance at least 2048 / 2 + 1 samples"""
    ps = [S.pair(RAGGED_SEEDS[j], L, S.SHAPES[j], 2048) for j, L in enumerate(RAGGED_LENS)]
    return [p[0] for p in ps], [p[1] for p in ps]


def floored_signals(case):
    """signals(case) with the middle x scaled until every bin of it lies below the floor (p_x < 1e-10 / 4) without being zero: the gradient of that
    utterance is exactly zero, which the mutant that passes a gradient through the floor does not give"""
    xs, ys = signals(case)
    xs[1] = (xs[1].astype(np.float64) * 1e-9).astype(np.float32)
    return xs, ys


def quiet_signals(case, scale=5e-5):
    """signals(case) with the middle pair scaled down: most of its bins lie between the mel loss's floor 1e-10 and the STFT loss's 1e-7, so a floor
    at 1e-7 changes its mels"""
    xs, ys = signals(case)
    xs[1], ys[1] = (xs[1].astype(np.float64) * scale).astype(np.float32), (ys[1].astype(np.float64) * scale).astype(np.float32)
    return xs, ys


def symmetric_window(case):
    return F.symmetric_hann(case[2], case[0])


# ---- the same loss as torch.stft + matmul + log10 + autograd --------------------------------------------------------------------------------------
def torch_statement(xs, ys, cases, reduction, g=1.0, dtype=None, bases=None, detail=False):
    """(loss, per-utterance gradient of g loss) on the CPU in `dtype` (float64 by default); detail: also, per resolution, the per-frame sums [frames]"""
    import torch

    dtype = torch.float64 if dtype is None else dtype
    tx = [torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True) for x in xs]
    ty = [torch.tensor(np.asarray(y), dtype=dtype) for y in ys]
    vals, frames = [], []
    for i, case in enumerate(cases):
        n_fft, hop, wl = case[:3]
        B = torch.tensor(np.asarray(filterbank(case) if bases is None else bases[i]), dtype=dtype)
        win = torch.hann_window(wl, dtype=dtype)
        per = []
        for x, y in zip(tx, ty):
            l = []
            for v in (x, y):
                Z = torch.stft(v, n_fft, hop, wl, win, center=True, pad_mode="reflect", return_complex=True).transpose(0, 1)
                m = torch.sqrt(torch.clamp(Z.real ** 2 + Z.imag ** 2, min=FLOOR))
                l.append(torch.log10(torch.clamp(m @ B.T, min=FLOOR)))
            per.append((l[0] - l[1]).abs())
        frames.append(np.concatenate([p.sum(1).detach().numpy() for p in per]))
        if reduction == "batch":
            vals.append(torch.nn.functional.l1_loss(torch.cat(per), torch.zeros_like(torch.cat(per))))
        else:
            vals.append(torch.stack([p.mean() for p in per]).mean())
    val = torch.stack(vals).mean()
    (g * val).backward()
    out = (float(val.detach()), [x.grad.numpy().astype(np.float64) for x in tx])
    return out + (frames,) if detail else out
