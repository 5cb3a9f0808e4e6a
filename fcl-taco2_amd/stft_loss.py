"""Multi-resolution STFT loss on the HIP path: spectral convergence and log-magnitude distance of a generated waveform against a target, with the
gradient with respect to the generated one (csrc/stft_loss.hip).

The validation figure and generator loss of Parallel WaveGAN (`parallel_wavegan.losses.MultiResolutionSTFTLoss`): per resolution (n_fft, hop,
win_length), on reflect-padded centred frames under a periodic Hann window, m = sqrt(max(re^2 + im^2, 1e-7)) for both signals,
sc = sqrt(sum (m_y - m_x)^2 / sum m_y^2) and mag = mean |log m_y - log m_x|; the module returns the means over the resolutions.  The contract is
stated in include/fcl_hip.h "Multi-resolution STFT loss" and restated in float64 numpy in tests/stft_loss_ref.py.

    loss = MultiResolutionSTFTLoss("cuda:0")
    sc, mag = loss(generator(z), target)        # [B, T], [B, 1, T] or packed 1-D with lens=
    (sc + mag).backward()

An utterance of L samples needs L >= n_fft / 2 + 1 of the largest resolution.  Spectra never reach memory: the backward pass recomputes both
transforms.  No CPU fallback."""
import ctypes as C

import numpy as np
import torch

from . import _lib, features, griffinlim, ops

FFT_SIZES, HOP_SIZES, WIN_LENGTHS = (1024, 2048, 512), (120, 240, 50), (600, 1200, 240)  # Parallel WaveGAN's
MAX_RESOLUTIONS = 8
REDUCTIONS = ("batch", "utterance")


def check_resolutions(fft_sizes, hop_sizes, win_lengths):
    """One to eight resolutions, three lists of one length, each (n_fft, hop, win_length) what the kernels cover (griffinlim.check_config);
    anything else is refused by name before the first device call."""
    fft_sizes, hop_sizes, win_lengths = list(fft_sizes), list(hop_sizes), list(win_lengths)
    if not (len(fft_sizes) == len(hop_sizes) == len(win_lengths)):
        raise ValueError("fcl-taco2_amd: STFT loss: fft sizes, hops and window lengths must have one length (got %d, %d, %d)"
                         % (len(fft_sizes), len(hop_sizes), len(win_lengths)))
    if not 1 <= len(fft_sizes) <= MAX_RESOLUTIONS:
        raise ValueError("fcl-taco2_amd: STFT loss: 1 .. %d resolutions expected (got %d)" % (MAX_RESOLUTIONS, len(fft_sizes)))
    for n, h, w in zip(fft_sizes, hop_sizes, win_lengths):
        griffinlim.check_config(int(n), int(h), int(w))
    return [(int(n), int(h), int(w)) for n, h, w in zip(fft_sizes, hop_sizes, win_lengths)]


class Resolution(object):
    """One resolution's device tables"""

    def __init__(self, n_fft, hop, win_length, dev):
        self.n_fft, self.hop, self.win_length, self.bins = n_fft, hop, win_length, n_fft // 2 + 1
        self.window = griffinlim.hann_window(win_length, n_fft)
        self.window_d = torch.from_numpy(np.ascontiguousarray(self.window, dtype=np.float32)).to(dev)
        self.twiddle_d = torch.from_numpy(griffinlim.twiddles(n_fft)).to(dev)


class STFTLossPlan(object):
    """Configuration and device tables: per resolution the window (periodic Hann of win_length, zero-padded centred to n_fft) and the twiddles."""

    def __init__(self, device, fft_sizes=FFT_SIZES, hop_sizes=HOP_SIZES, win_lengths=WIN_LENGTHS):
        self.configs = check_resolutions(fft_sizes, hop_sizes, win_lengths)
        if not str(device).startswith("cuda"):
            raise _lib.FclError("fcl-taco2_amd: STFTLossPlan needs a GPU device (no CPU fallback)")
        self.device = dev = torch.device(device)
        with torch.cuda.device(dev):
            self.resolutions = [Resolution(n, h, w, dev) for n, h, w in self.configs]
        self.max_n_fft = max(n for n, _, _ in self.configs)

    def check_lens(self, lens, ids=None):
        """every utterance needs max n_fft / 2 + 1 samples; the first shorter one is refused by id"""
        features.check_lens(lens, self.max_n_fft, ids)


Maps = features.Maps  # frame_utt / utt_off / smp_off of a batch from its sample counts


def _args(rs, mp, x, y, **ptr):
    a = _lib.StftLoss()
    a.frames, a.samples, a.n_fft, a.hop, a.n_utt, a.accumulate = mp.frames, mp.samples, rs.n_fft, rs.hop, mp.n_utt, 0
    a.x, a.y, a.smp_off, a.frame_utt, a.utt_off = x.data_ptr(), y.data_ptr(), mp.smp_off.data_ptr(), mp.frame_utt.data_ptr(), mp.utt_off.data_ptr()
    a.window, a.twiddle = rs.window_d.data_ptr(), rs.twiddle_d.data_ptr()
    for k, v in ptr.items():
        setattr(a, k, v.data_ptr())
    return a


# two launches each, on caller-owned buffers (the tests surround them with guard zones)
def launch_sums(rs, mp, x, y, frame_sums, utt_sums):
    """x, y [samples] float32 -> frame_sums [frames, 3] float32, utt_sums [n_utt, 3] float64: (sum (m_y - m_x)^2, sum m_y^2, sum |log m_y - log m_x|)"""
    _lib.check(_lib.load().fcl_stl_sums_fwd(C.byref(_args(rs, mp, x, y, frame_sums=frame_sums, utt_sums=utt_sums)), ops._stream()))


def launch_grad(rs, mp, x, y, coef, fr, gx, accumulate=False):
    """coef [n_utt, 2] float32 = (-g_sc / sqrt(A B), g_mag / n) per utterance; fr [frames, n_fft] float32 scratch -> gx [samples] float32
    (accumulate: added to gx)"""
    a = _args(rs, mp, x, y, coef=coef, fr=fr, gx=gx)
    a.accumulate = int(bool(accumulate))
    _lib.check(_lib.load().fcl_stl_grad_bwd(C.byref(a), ops._stream()))


def _figures(sums, n, reduction):
    """sums [n_utt, 3] float64 on the device, n [n_utt] float64 (frames x bins) -> (sc, mag) float64 scalars of one resolution"""
    if reduction == "batch":
        tot = sums.sum(0)
        return torch.sqrt(tot[0] / tot[1]), tot[2] / n.sum()
    return torch.sqrt(sums[:, 0] / sums[:, 1]).mean(), (sums[:, 2] / n).mean()


class _Function(torch.autograd.Function):
    """(sc, mag) of packed x against packed y: the sums of every resolution forward, the gradient launches backward; y gets no gradient"""

    @staticmethod
    def forward(ctx, x, y, plan, maps, ns, reduction):
        dev = plan.device
        with torch.cuda.device(dev):
            x, y = x.detach(), y.detach()
            all_sums, sc, mag = [], 0.0, 0.0
            for rs, mp, n in zip(plan.resolutions, maps, ns):
                frame_sums = torch.empty(mp.frames, 3, device=dev, dtype=torch.float32)
                utt_sums = torch.empty(mp.n_utt, 3, device=dev, dtype=torch.float64)
                launch_sums(rs, mp, x, y, frame_sums, utt_sums)
                s, m = _figures(utt_sums, n, reduction)
                sc, mag = sc + s, mag + m
                all_sums.append(utt_sums)
            R = len(plan.resolutions)
        ctx.plan, ctx.maps, ctx.ns, ctx.reduction = plan, maps, ns, reduction
        ctx.save_for_backward(x, y, *all_sums)
        return (sc / R).to(torch.float32), (mag / R).to(torch.float32)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_sc, g_mag):
        plan, dev = ctx.plan, ctx.plan.device
        x, y = ctx.saved_tensors[:2]
        R = len(plan.resolutions)
        with torch.cuda.device(dev):
            zero = torch.zeros((), device=dev, dtype=torch.float64)
            g_sc = (zero if g_sc is None else g_sc.to(torch.float64)) / R
            g_mag = (zero if g_mag is None else g_mag.to(torch.float64)) / R
            gx = torch.empty_like(x)
            for i, (rs, mp, n, sums) in enumerate(zip(plan.resolutions, ctx.maps, ctx.ns, ctx.saved_tensors[2:])):
                if ctx.reduction == "batch":
                    tot = sums.sum(0)
                    c0 = (-g_sc / torch.sqrt(tot[0] * tot[1])).expand(mp.n_utt)
                    c1 = (g_mag / n.sum()).expand(mp.n_utt)
                else:
                    c0 = -g_sc / torch.sqrt(sums[:, 0] * sums[:, 1]) / mp.n_utt
                    c1 = g_mag / n / mp.n_utt
                coef = torch.stack([c0, c1], dim=1).to(torch.float32).contiguous()
                fr = torch.empty(mp.frames, rs.n_fft, device=dev, dtype=torch.float32)
                launch_grad(rs, mp, x, y, coef, fr, gx, accumulate=i > 0)
        return gx, None, None, None, None, None


class MultiResolutionSTFTLoss(torch.nn.Module):
    """forward(x, y, lens=None, reduction="batch") -> (sc, mag): float32 scalars on the device, each the mean over the resolutions.

    x (generated) and y (target): [B, T], [B, 1, T], or 1-D packed (utterances back to back) with lens.  lens with a 2-D input: row b counts its first
    lens[b] samples, the padding gets zero gradient.  reduction "batch": one set of sums over all frames of the batch (for equal-length clips what
    `parallel_wavegan.losses.MultiResolutionSTFTLoss` computes); "utterance": per-utterance figures, their mean over the utterances."""

    def __init__(self, device="cuda:0", fft_sizes=FFT_SIZES, hop_sizes=HOP_SIZES, win_lengths=WIN_LENGTHS, plan=None):
        super().__init__()
        self.plan = STFTLossPlan(device, fft_sizes, hop_sizes, win_lengths) if plan is None else plan
        self._maps_key, self._maps = None, None

    def maps(self, lens):
        """the batch's maps per resolution and n = frames x bins per utterance (float64, on the device); kept for the next batch of the same lengths"""
        key = tuple(lens)
        if key != self._maps_key:
            pl, dev = self.plan, self.plan.device
            with torch.cuda.device(dev):
                mps = [Maps(lens, rs.hop, dev) for rs in pl.resolutions]
                ns = [torch.tensor([t * rs.bins for t in mp.lens], dtype=torch.float64).to(dev) for rs, mp in zip(pl.resolutions, mps)]
            for rs, mp in zip(pl.resolutions, mps):
                if mp.samples >= 2 ** 31 - 1 or mp.frames * rs.n_fft >= 2 ** 31 - 1:
                    raise _lib.FclError("fcl-taco2_amd: more than 2^31 samples or frames x n_fft in one STFT-loss batch")
            self._maps_key, self._maps = key, (mps, ns)
        return self._maps

    def pack(self, x, y, lens=None, ids=None):
        """-> (x packed, y packed, lens) on the plan's device in float32; the packing is made of torch operations, so a gradient flows back through it"""
        dev = self.plan.device
        x, y = torch.as_tensor(x), torch.as_tensor(y)
        if tuple(x.shape) != tuple(y.shape):
            raise ValueError("fcl-taco2_amd: STFT loss: x is %r, y is %r" % (tuple(x.shape), tuple(y.shape)))
        if x.dim() == 3:
            if x.shape[1] != 1:
                raise ValueError("fcl-taco2_amd: STFT loss: a 3-D input must be [B, 1, T], got %r" % (tuple(x.shape),))
            x, y = x[:, 0], y[:, 0]
        x, y = x.to(device=dev, dtype=torch.float32), y.to(device=dev, dtype=torch.float32)
        if x.dim() == 1:
            if lens is None:
                lens = [int(x.numel())]
            lens = [int(n) for n in lens]
            if sum(lens) != x.numel():
                raise ValueError("fcl-taco2_amd: STFT loss: the packed waveform has %d samples, lens sum to %d" % (x.numel(), sum(lens)))
        elif x.dim() == 2:
            B, T = x.shape
            if lens is None:
                lens = [int(T)] * int(B)
                x, y = x.reshape(-1), y.reshape(-1)
            else:
                lens = [int(n) for n in lens]
                if len(lens) != B or max(lens) > T or min(lens) < 0:
                    raise ValueError("fcl-taco2_amd: STFT loss: lens %r do not fit an input of %r" % (lens, tuple(x.shape)))
                x, y = torch.cat([x[b, :n] for b, n in enumerate(lens)]), torch.cat([y[b, :n] for b, n in enumerate(lens)])
        else:
            raise ValueError("fcl-taco2_amd: STFT loss: [B, T], [B, 1, T] or packed 1-D input expected, got %r" % (tuple(x.shape),))
        self.plan.check_lens(lens, ids)
        return x.contiguous(), y.contiguous(), lens

    def forward(self, x, y, lens=None, reduction="batch", ids=None):
        if reduction not in REDUCTIONS:
            raise ValueError("fcl-taco2_amd: STFT loss: reduction %r is not one of %r" % (reduction, REDUCTIONS))
        if torch.is_tensor(y) and y.requires_grad:
            raise ValueError("fcl-taco2_amd: STFT loss: y (the target) must not require a gradient: only x gets one")
        x, y, lens = self.pack(x, y, lens, ids)
        mps, ns = self.maps(lens)
        return _Function.apply(x, y, self.plan, mps, ns, reduction)

    def distances(self, x, lens, y, ids=None):
        """packed x, y (or lists of 1-D waveforms; lens is then ignored) -> (sc [n_utt, R], mag [n_utt, R]) float64 numpy: every utterance's own figures
        per resolution, for the evaluation driver"""
        if isinstance(x, (list, tuple)):
            lens = [int(np.asarray(v).shape[0]) for v in x]
            x, y = np.concatenate([np.asarray(v, dtype=np.float32) for v in x]), np.concatenate([np.asarray(v, dtype=np.float32) for v in y])
        with torch.no_grad():
            x, y, lens = self.pack(x, y, lens, ids)
        mps, ns = self.maps(lens)
        dev = self.plan.device
        sc, mag = [], []
        with torch.cuda.device(dev):
            for rs, mp, n in zip(self.plan.resolutions, mps, ns):
                frame_sums = torch.empty(mp.frames, 3, device=dev, dtype=torch.float32)
                utt_sums = torch.empty(mp.n_utt, 3, device=dev, dtype=torch.float64)
                launch_sums(rs, mp, x, y, frame_sums, utt_sums)
                sc.append(torch.sqrt(utt_sums[:, 0] / utt_sums[:, 1]))
                mag.append(utt_sums[:, 2] / n)
            return torch.stack(sc, 1).cpu().numpy(), torch.stack(mag, 1).cpu().numpy()


def distances(x, lens, y, device="cuda:0", fft_sizes=FFT_SIZES, hop_sizes=HOP_SIZES, win_lengths=WIN_LENGTHS, ids=None):
    """per-utterance, per-resolution (sc, mag) of packed x against packed y with a plan made for the call"""
    return MultiResolutionSTFTLoss(device, fft_sizes, hop_sizes, win_lengths).distances(x, lens, y, ids=ids)


def add_arguments(g):
    """The drivers' resolution flags; the defaults are Parallel WaveGAN's."""
    ints = lambda s: [int(v) for v in s.replace(",", " ").split()]
    g.add_argument("--stft-fft-sizes", type=ints, default=list(FFT_SIZES), metavar="N,N,..", help="n_fft per resolution (512, 1024 or 2048 each)")
    g.add_argument("--stft-hops", type=ints, default=list(HOP_SIZES), metavar="H,H,..", help="hop per resolution")
    g.add_argument("--stft-win-lengths", type=ints, default=list(WIN_LENGTHS), metavar="W,W,..", help="window length per resolution")
