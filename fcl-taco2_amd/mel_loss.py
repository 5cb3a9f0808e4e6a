"""Mel-spectrogram L1 loss on the HIP path: the distance of the log10 mel spectrograms of a generated waveform and a target, with the gradient with
respect to the generated one (the msl_* kernels of csrc/stft_loss.hip).

HiFi-GAN's reconstruction term (weight 45 beside the adversarial terms) and the usual loss for fine-tuning a generator on an acoustic model's own
mels.  Per resolution (n_fft, hop, win_length, mel matrix B), on the frames of stft_loss.py: m = sqrt(max(re^2 + im^2, 1e-10)) for both signals,
M_c = max(sum_k m_k B[c, k], 1e-10), l_c = log10 M_c, and the loss is the mean of |l_x - l_y| over frames and channels; the module returns the mean
over the resolutions.  With the defaults -- the single resolution of features.DEFAULTS -- the mel is the one features.py extracts and FCL-taco2
predicts.  The contract is stated in include/fcl_hip.h "Mel-spectrogram loss" and restated in float64 numpy in tests/mel_loss_ref.py.

    mel = MelSpectrogramLoss("cuda:0")
    (45 * mel(generator(z), target)).backward()        # [B, T], [B, 1, T] or packed 1-D with lens=

An utterance of L samples needs L >= n_fft / 2 + 1 of the largest resolution.  Spectra and mels never reach memory: the backward pass recomputes
them.  No CPU fallback."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib, features, griffinlim, ops, stft_loss

D = features.DEFAULTS
REDUCTIONS = stft_loss.REDUCTIONS
Maps = features.Maps


def bin_major_transpose(fb_lo, fb_off, fb_w, bins):
    """the banded filterbank listed by bin -> (bt_off [bins + 1], bt_ch [nnz], bt_w [nnz]): bin k is covered by the channels bt_ch[bt_off[k] ..
    bt_off[k + 1]) in ascending order with the weights bt_w.  A list, not a run: the channels that cover a bin need not be contiguous."""
    per = [[] for _ in range(bins)]
    for c, a in enumerate(fb_lo):
        for j in range(int(fb_off[c]), int(fb_off[c + 1])):
            per[int(a) + j - int(fb_off[c])].append((c, fb_w[j]))
    off = np.concatenate([[0], np.cumsum([len(p) for p in per])]).astype(np.int32)
    return off, np.asarray([c for p in per for c, _ in p], dtype=np.int32), np.asarray([w for p in per for _, w in p], dtype=np.asarray(fb_w).dtype)


def dense_from_transpose(bt_off, bt_ch, bt_w, n_mels):
    """the inverse of bin_major_transpose, as a dense [n_mels, bins] matrix"""
    B = np.zeros((n_mels, len(bt_off) - 1), dtype=np.asarray(bt_w).dtype)
    for k in range(len(bt_off) - 1):
        B[bt_ch[bt_off[k] : bt_off[k + 1]], k] = bt_w[bt_off[k] : bt_off[k + 1]]
    return B


class Resolution(stft_loss.Resolution):
    """One resolution's device tables: window and twiddles, the banded filterbank and its bin-major transpose"""

    def __init__(self, n_fft, hop, win_length, B, dev):
        stft_loss.Resolution.__init__(self, n_fft, hop, win_length, dev)
        self.B, self.n_mels = B, int(B.shape[0])
        self.fb_lo, self.fb_off, self.fb_w = features.banded_filterbank(B)
        self.bt_off, self.bt_ch, self.bt_w = bin_major_transpose(self.fb_lo, self.fb_off, self.fb_w, self.bins)
        self.nnz = int(len(self.fb_w))
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
        self.fb_lo_d, self.fb_off_d, self.fb_w_d = t(self.fb_lo, np.int32), t(self.fb_off, np.int32), t(self.fb_w, np.float32)
        self.bt_off_d, self.bt_ch_d, self.bt_w_d = t(self.bt_off, np.int32), t(self.bt_ch, np.int32), t(self.bt_w, np.float32)


def check_configuration(fs, fft_sizes, hop_sizes, win_lengths, n_mels, fmin, fmax, mel_bases=None):
    """-> [(n_fft, hop, win_length, B)]: one to eight resolutions the kernels cover (griffinlim.check_config), each with its mel matrix -- the
    Slaney one of (fs, n_mels, fmin, fmax) or the caller's -- of contiguous bands (features.banded_filterbank); anything else is refused by name."""
    fft_sizes, win_lengths = list(fft_sizes), list(win_lengths)
    if len(win_lengths) == len(fft_sizes):
        win_lengths = [n if w is None else w for n, w in zip(fft_sizes, win_lengths)]  # None: n_fft, as the drivers' --win-length
    configs = stft_loss.check_resolutions(fft_sizes, hop_sizes, win_lengths)
    if mel_bases is not None and len(mel_bases) != len(configs):
        raise ValueError("fcl-taco2_amd: mel loss: %d mel bases for %d resolutions" % (len(mel_bases), len(configs)))
    out = []
    for i, (n, h, w) in enumerate(configs):
        if mel_bases is not None and mel_bases[i] is not None:
            B = np.asarray(mel_bases[i], dtype=np.float64)
            if B.ndim != 2 or B.shape[1] != n // 2 + 1:
                raise ValueError("fcl-taco2_amd: mel loss: mel_basis %d must be [n_mels, %d] for n_fft %d, got shape %r" % (i, n // 2 + 1, n, B.shape))
            griffinlim.check_config(n, h, w, int(B.shape[0]), fs, fmin, fmax)
        else:
            griffinlim.check_config(n, h, w, int(n_mels), fs, fmin, fmax)
            B = griffinlim.mel_filterbank(fs, n, int(n_mels), float(fmin), float(fmax))
        features.banded_filterbank(B)
        out.append((n, h, w, B))
    return out


class MelLossPlan(object):
    """Configuration and device tables; the defaults are the single resolution of features.DEFAULTS.  mel_bases: per resolution a [n_mels, bins]
    matrix replacing the built Slaney one (or None)."""

    def __init__(self, device, fs=D["fs"], fft_sizes=(D["n_fft"],), hop_sizes=(D["hop"],), win_lengths=(D["win_length"],), n_mels=D["n_mels"],
                 fmin=D["fmin"], fmax=D["fmax"], mel_bases=None):
        cfg = check_configuration(fs, fft_sizes, hop_sizes, win_lengths, n_mels, fmin, fmax, mel_bases)
        self.configs = [c[:3] for c in cfg]
        self.fs, self.fmin, self.fmax = int(fs), float(fmin), float(fmax)
        if not str(device).startswith("cuda"):
            raise _lib.FclError("fcl-taco2_amd: MelLossPlan needs a GPU device (no CPU fallback)")
        self.device = dev = torch.device(device)
        with torch.cuda.device(dev):
            self.resolutions = [Resolution(n, h, w, B, dev) for n, h, w, B in cfg]
        self.max_n_fft = max(c[0] for c in self.configs)

    def check_lens(self, lens, ids=None):
        """every utterance needs max n_fft / 2 + 1 samples; the first shorter one is refused by id"""
        features.check_lens(lens, self.max_n_fft, ids)


def _args(rs, mp, x, y, **ptr):
    a = _lib.MelLoss()
    a.frames, a.samples, a.n_fft, a.hop, a.n_utt, a.accumulate, a.n_mels, a.nnz = mp.frames, mp.samples, rs.n_fft, rs.hop, mp.n_utt, 0, rs.n_mels, rs.nnz
    a.x, a.y, a.smp_off, a.frame_utt, a.utt_off = x.data_ptr(), y.data_ptr(), mp.smp_off.data_ptr(), mp.frame_utt.data_ptr(), mp.utt_off.data_ptr()
    a.window, a.twiddle = rs.window_d.data_ptr(), rs.twiddle_d.data_ptr()
    a.fb_lo, a.fb_off, a.fb_w = rs.fb_lo_d.data_ptr(), rs.fb_off_d.data_ptr(), rs.fb_w_d.data_ptr()
    a.bt_off, a.bt_ch, a.bt_w = rs.bt_off_d.data_ptr(), rs.bt_ch_d.data_ptr(), rs.bt_w_d.data_ptr()
    for k, v in ptr.items():
        setattr(a, k, v.data_ptr())
    return a


# on caller-owned buffers (the tests surround them with guard zones)
def launch_sums(rs, mp, x, y, frame_sums, utt_sums):
    """x, y [samples] float32 -> frame_sums [frames] float32, utt_sums [n_utt] float64: sum over the channels (and frames) of |l_x - l_y|"""
    _lib.check(_lib.load().fcl_msl_sums_fwd(C.byref(_args(rs, mp, x, y, frame_sums=frame_sums, utt_sums=utt_sums)), ops._stream()))


def launch_grad(rs, mp, x, y, coef, fr, gx, accumulate=False):
    """coef [n_utt] float32 = g / (ln 10 n) per utterance; fr [frames, n_fft] float32 scratch -> gx [samples] float32 (accumulate: added to gx)"""
    a = _args(rs, mp, x, y, coef=coef, fr=fr, gx=gx)
    a.accumulate = int(bool(accumulate))
    _lib.check(_lib.load().fcl_msl_grad_bwd(C.byref(a), ops._stream()))


class _Function(torch.autograd.Function):
    """the loss of packed x against packed y: the sums of every resolution forward, the gradient launches backward; y gets no gradient"""

    @staticmethod
    def forward(ctx, x, y, plan, maps, ns, reduction):
        dev = plan.device
        with torch.cuda.device(dev):
            x, y = x.detach(), y.detach()
            loss = 0.0
            for rs, mp, n in zip(plan.resolutions, maps, ns):
                frame_sums = torch.empty(mp.frames, device=dev, dtype=torch.float32)
                utt_sums = torch.empty(mp.n_utt, device=dev, dtype=torch.float64)
                launch_sums(rs, mp, x, y, frame_sums, utt_sums)
                loss = loss + (utt_sums.sum() / n.sum() if reduction == "batch" else (utt_sums / n).mean())
        ctx.plan, ctx.maps, ctx.ns, ctx.reduction = plan, maps, ns, reduction
        ctx.save_for_backward(x, y)
        return (loss / len(plan.resolutions)).to(torch.float32)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        plan, dev = ctx.plan, ctx.plan.device
        x, y = ctx.saved_tensors
        with torch.cuda.device(dev):
            g = g.to(torch.float64) / (len(plan.resolutions) * math.log(10.0))
            gx = torch.empty_like(x)
            for i, (rs, mp, n) in enumerate(zip(plan.resolutions, ctx.maps, ctx.ns)):
                coef = ((g / n.sum()).expand(mp.n_utt) if ctx.reduction == "batch" else g / n / mp.n_utt).to(torch.float32).contiguous()
                fr = torch.empty(mp.frames, rs.n_fft, device=dev, dtype=torch.float32)
                launch_grad(rs, mp, x, y, coef, fr, gx, accumulate=i > 0)
        return gx, None, None, None, None, None


class MelSpectrogramLoss(torch.nn.Module):
    """forward(x, y, lens=None, reduction="batch", ids=None) -> the loss: a float32 scalar on the device, the mean over the resolutions.

    x (generated) and y (target) as MultiResolutionSTFTLoss takes them: [B, T], [B, 1, T], or 1-D packed with lens; lens with a 2-D input: row b
    counts its first lens[b] samples, the padding gets zero gradient.  reduction "batch": the mean over all frames and channels of the batch (for
    equal-length clips F.l1_loss of the two log-mel tensors); "utterance": the mean of the per-utterance means."""

    def __init__(self, device="cuda:0", fs=D["fs"], fft_sizes=(D["n_fft"],), hop_sizes=(D["hop"],), win_lengths=(D["win_length"],), n_mels=D["n_mels"],
                 fmin=D["fmin"], fmax=D["fmax"], mel_bases=None, plan=None):
        super().__init__()
        self.plan = MelLossPlan(device, fs, fft_sizes, hop_sizes, win_lengths, n_mels, fmin, fmax, mel_bases) if plan is None else plan
        self._maps_key, self._maps = None, None

    def maps(self, lens):
        """the batch's maps per resolution and n = frames x n_mels per utterance (float64, on the device); kept for the next batch of the same lengths"""
        key = tuple(lens)
        if key != self._maps_key:
            pl, dev = self.plan, self.plan.device
            with torch.cuda.device(dev):
                mps = [Maps(lens, rs.hop, dev) for rs in pl.resolutions]
                ns = [torch.tensor([t * rs.n_mels for t in mp.lens], dtype=torch.float64).to(dev) for rs, mp in zip(pl.resolutions, mps)]
            for rs, mp in zip(pl.resolutions, mps):
                if mp.samples >= 2 ** 31 - 1 or mp.frames * rs.n_fft >= 2 ** 31 - 1:
                    raise _lib.FclError("fcl-taco2_amd: more than 2^31 samples or frames x n_fft in one mel-loss batch")
            self._maps_key, self._maps = key, (mps, ns)
        return self._maps

    pack = stft_loss.MultiResolutionSTFTLoss.pack  # the same input forms, the same packing

    def forward(self, x, y, lens=None, reduction="batch", ids=None):
        if reduction not in REDUCTIONS:
            raise ValueError("fcl-taco2_amd: mel loss: reduction %r is not one of %r" % (reduction, REDUCTIONS))
        if torch.is_tensor(y) and y.requires_grad:
            raise ValueError("fcl-taco2_amd: mel loss: y (the target) must not require a gradient: only x gets one")
        x, y, lens = self.pack(x, y, lens, ids)
        mps, ns = self.maps(lens)
        return _Function.apply(x, y, self.plan, mps, ns, reduction)

    def distances(self, x, lens, y, ids=None):
        """packed x, y (or lists of 1-D waveforms; lens is then ignored) -> [n_utt, R] float64 numpy: every utterance's own mel-L1 per resolution,
        for the evaluation driver"""
        if isinstance(x, (list, tuple)):
            lens = [int(np.asarray(v).shape[0]) for v in x]
            x, y = np.concatenate([np.asarray(v, dtype=np.float32) for v in x]), np.concatenate([np.asarray(v, dtype=np.float32) for v in y])
        with torch.no_grad():
            x, y, lens = self.pack(x, y, lens, ids)
        mps, ns = self.maps(lens)
        dev = self.plan.device
        out = []
        with torch.cuda.device(dev):
            for rs, mp, n in zip(self.plan.resolutions, mps, ns):
                frame_sums = torch.empty(mp.frames, device=dev, dtype=torch.float32)
                utt_sums = torch.empty(mp.n_utt, device=dev, dtype=torch.float64)
                launch_sums(rs, mp, x, y, frame_sums, utt_sums)
                out.append(utt_sums / n)
            return torch.stack(out, 1).cpu().numpy()


def distances(x, lens, y, device="cuda:0", ids=None, **config):
    """per-utterance, per-resolution mel-L1 of packed x against packed y with a plan made for the call"""
    return MelSpectrogramLoss(device, **config).distances(x, lens, y, ids=ids)


def from_args(args, device):
    """the loss on a driver's parsed analysis flags (griffinlim.add_analysis_arguments, --n-mels, --mel-basis): the mel of features.from_args"""
    basis = None if args.mel_basis is None else [np.load(args.mel_basis)]
    return MelSpectrogramLoss(device, args.fs, [args.n_fft], [args.hop], [args.win_length], args.n_mels, args.fmin, args.fmax, basis)
