"""Griffin-Lim vocoder on the HIP path: mel [T', n_mels] -> waveform [hop * (T' - 1)] with no trained generator (csrc/griffinlim.hip).

The route ESPnet's recipes take before a neural vocoder exists: de-normalise (mel_stats.npy of preprocess.py:130-141), 10^x, pseudo-inverse of the mel
filterbank, Griffin-Lim with momentum.  Every constant comes from the reference's preprocess.py (lines 40-50, 71: log10 mel of an STFT magnitude,
n_fft 1024, hop 256, Hann, 80 mels over 80 - 7600 Hz at 22.05 kHz).  The algorithm is stated in include/fcl_hip.h and restated in float64 numpy in
tests/griffinlim_ref.py; ESPnet's source is not available here, so that statement is the contract (DESIGN §6d names the rule it would have to confirm).

`GriffinLim` has the generators' surface (`plan.hop`, `plan.A`, `plan.device`, `plan.eager_only`, `synthesize_packed`, `synthesize`, `inference`,
`samples_of`); an utterance of T frames gives hop * (T - 1) samples.  There is no capacity form: tts.synthesize takes the two-step route for every
batch.  No CPU fallback."""
import ctypes as C

import numpy as np
import torch

from . import _lib, ops
from .vocoder import Generator

DEFAULTS = dict(fs=22050, n_fft=1024, hop=256, win_length=None, n_mels=80, fmin=80.0, fmax=7600.0, n_iter=64, momentum=0.99)  # preprocess.py's analysis
N_FFTS = (512, 1024, 2048)


# ---- host-side tables (float64 numpy) -----------------------------------------------------------------------------------------------------------
def hz_to_mel(f):
    """Slaney mel scale: linear below 1 kHz (200 / 3 Hz per mel), logarithmic above (27 mels per factor 6.4)"""
    f = np.asarray(f, dtype=np.float64)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) * (27.0 / np.log(6.4)), f * (3.0 / 200.0))


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((m - 15.0) * (np.log(6.4) / 27.0)), m * (200.0 / 3.0))


def mel_filterbank(fs, n_fft, n_mels, fmin, fmax):
    """B [n_mels, n_fft / 2 + 1]: triangular filters between n_mels + 2 edges equally spaced on the Slaney mel scale, each scaled by 2 / (f_hi - f_lo)"""
    edges = mel_to_hz(np.linspace(float(hz_to_mel(fmin)), float(hz_to_mel(fmax)), n_mels + 2))
    freqs = np.linspace(0.0, fs / 2.0, n_fft // 2 + 1)
    lower = (freqs[None, :] - edges[:-2, None]) / (edges[1:-1] - edges[:-2])[:, None]
    upper = (edges[2:, None] - freqs[None, :]) / (edges[2:] - edges[1:-1])[:, None]
    return np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (edges[2:] - edges[:-2]))[:, None]


def hann_window(win_length, n_fft):
    """periodic Hann of win_length, zero-padded centred to n_fft"""
    out = np.zeros(n_fft)
    lp = (n_fft - win_length) // 2
    out[lp : lp + win_length] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win_length) / win_length)
    return out


def window_sumsquare(window, hop, frames):
    """[n_fft + hop (frames - 1)]: what the overlap-add divides by (where it exceeds FLT_MIN)"""
    n_fft = len(window)
    wss = np.zeros(n_fft + hop * (frames - 1))
    for t in range(frames):
        wss[t * hop : t * hop + n_fft] += np.asarray(window, dtype=np.float64) ** 2
    return wss


def twiddles(n_fft):
    """[n_fft, 2] float32: exp(-2 pi i k / n_fft) computed in double, the axis values exact"""
    k = np.arange(n_fft)
    w = np.stack([np.cos(2.0 * np.pi * k / n_fft), -np.sin(2.0 * np.pi * k / n_fft)], axis=1)
    for q, v in ((0, (1.0, 0.0)), (n_fft // 4, (0.0, -1.0)), (n_fft // 2, (-1.0, 0.0)), (3 * n_fft // 4, (0.0, 1.0))):
        w[q] = v
    return np.ascontiguousarray(w, dtype=np.float32)


def _hash_u32(x):
    x = np.asarray(x, dtype=np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def phase_uniforms(utt_seed, frames, bins):
    """numpy twin of the device's draw (fcl_gl_phase_init): u [frames, bins] float32 in [0, 1) of one utterance,
    u = (h(h(seed ^ h(t + 0x9E3779B9)) ^ (k * 0x85EBCA6B)) >> 8) * 2^-24 in wrapping uint32 arithmetic; the initial phase is exp(2 pi i u)."""
    with np.errstate(over="ignore"):
        a = _hash_u32(np.uint32(int(utt_seed) & 0xFFFFFFFF) ^ _hash_u32(np.arange(frames, dtype=np.uint32) + np.uint32(0x9E3779B9)))
        h = _hash_u32(a[:, None] ^ (np.arange(bins, dtype=np.uint32) * np.uint32(0x85EBCA6B))[None, :])
    return (h >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def min_frames(n_fft, hop):
    """the shortest utterance: T >= n_fft / (2 hop) + 2, so that the reflection at either end is a single one"""
    return -(-int(n_fft) // (2 * int(hop))) + 2


def check_config(n_fft, hop, win_length, n_mels=80, fs=22050, fmin=80.0, fmax=7600.0, n_iter=64, momentum=0.99):
    """What the kernels cover; anything else is refused by name (NotImplementedError / ValueError) before the first device call."""
    if n_fft not in N_FFTS:
        raise NotImplementedError("fcl-taco2_amd: Griffin-Lim: n_fft %r is not supported on the HIP path (n_fft must be one of %r)" % (n_fft, N_FFTS))
    if not 1 <= hop <= n_fft // 2:
        raise NotImplementedError("fcl-taco2_amd: Griffin-Lim: hop %r is not supported (1 <= hop <= n_fft / 2 = %d)" % (hop, n_fft // 2))
    if not 1 <= win_length <= n_fft:
        raise NotImplementedError("fcl-taco2_amd: Griffin-Lim: win_length %r is not supported (1 <= win_length <= n_fft = %d)" % (win_length, n_fft))
    if not 1 <= n_mels <= 256:
        raise NotImplementedError("fcl-taco2_amd: Griffin-Lim: n_mels %r is not supported (1 .. 256)" % (n_mels,))
    if not 0.0 <= fmin < fmax <= fs / 2.0:
        raise ValueError("fcl-taco2_amd: Griffin-Lim: 0 <= fmin < fmax <= fs / 2 expected (got fmin %r, fmax %r, fs %r)" % (fmin, fmax, fs))
    if n_iter < 0:
        raise ValueError("fcl-taco2_amd: Griffin-Lim: n_iter must not be negative (got %r)" % (n_iter,))
    if not 0.0 <= momentum <= 1.0:
        raise ValueError("fcl-taco2_amd: Griffin-Lim: momentum must lie in [0, 1] (got %r)" % (momentum,))


def check_lens(lens, n_fft, hop, ids=None):
    """Every utterance needs min_frames(n_fft, hop) frames; the first shorter one is refused by id (its position without ids)."""
    need = min_frames(n_fft, hop)
    for i, n in enumerate(lens):
        if int(n) < need:
            raise ValueError("fcl-taco2_amd: Griffin-Lim: utterance %s has %d frames; n_fft %d with hop %d needs at least %d (n_fft / (2 hop) + 2: a single "
                             "reflection at either end)" % (ids[i] if ids is not None else "#%d" % i, int(n), n_fft, hop, need))


class GriffinLimPlan(object):
    """Configuration and device tables: filterbank B, pinv(B)^T (float64 numpy, uploaded as float32), window, twiddles.  `mel_basis` ([n_mels, F]
    array) replaces the built filterbank; `mel_stats` ([2, n_mels]: mean, std) de-normalises the input."""

    eager_only = True  # no capacity form: tts.synthesize takes the two-step route for every batch

    def __init__(self, device, fs=22050, n_fft=1024, hop=256, win_length=None, n_mels=80, fmin=80.0, fmax=7600.0, n_iter=64, momentum=0.99, mel_stats=None,
                 mel_basis=None):
        win_length = int(n_fft if win_length is None else win_length)
        if mel_basis is not None:
            mel_basis = np.asarray(mel_basis, dtype=np.float64)
            if mel_basis.ndim != 2:
                raise ValueError("fcl-taco2_amd: Griffin-Lim: mel_basis must be a [n_mels, n_fft / 2 + 1] matrix, got shape %r" % (mel_basis.shape,))
            n_mels = int(mel_basis.shape[0])
        check_config(n_fft, hop, win_length, n_mels, fs, fmin, fmax, n_iter, momentum)
        self.fs, self.n_fft, self.hop, self.win_length, self.A = int(fs), int(n_fft), int(hop), win_length, int(n_mels)
        self.fmin, self.fmax, self.n_iter, self.momentum = float(fmin), float(fmax), int(n_iter), float(momentum)
        self.bins = self.n_fft // 2 + 1
        if mel_basis is not None and mel_basis.shape[1] != self.bins:
            raise ValueError("fcl-taco2_amd: Griffin-Lim: mel_basis has %d columns, n_fft %d needs %d" % (mel_basis.shape[1], self.n_fft, self.bins))
        if mel_stats is not None:
            mel_stats = np.asarray(mel_stats, dtype=np.float64)
            if mel_stats.shape != (2, self.A):
                raise ValueError("fcl-taco2_amd: Griffin-Lim: mel_stats must be [2, %d] (mean, std), got %r" % (self.A, mel_stats.shape))
        self.B = mel_filterbank(self.fs, self.n_fft, self.A, self.fmin, self.fmax) if mel_basis is None else mel_basis
        self.pinv = np.linalg.pinv(self.B)  # [F, n_mels], float64
        self.window = hann_window(self.win_length, self.n_fft)
        self.mel_stats = mel_stats
        if not str(device).startswith("cuda"):
            raise _lib.FclError("fcl-taco2_amd: GriffinLimPlan needs a GPU device (no CPU fallback)")
        self.device = dev = torch.device(device)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
        with torch.cuda.device(dev):
            self.pinv_t_d, self.window_d, self.twiddle_d = t(self.pinv.T), t(self.window), t(twiddles(self.n_fft))
            self.stats_d = None if mel_stats is None else t(mel_stats)

    def window_sumsquare(self, frames):
        return window_sumsquare(self.window, self.hop, frames)


class Maps(object):
    """frame_utt / utt_off of a batch on the device (as the other vocoder kernels take utterance bounds) and the sample offsets on the host"""

    def __init__(self, lens, dev):
        self.lens = [int(n) for n in lens]
        self.frames, self.n_utt = sum(self.lens), len(self.lens)
        offs = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)
        self.frame_utt = torch.from_numpy(np.repeat(np.arange(self.n_utt), self.lens).astype(np.int32)).to(dev)
        self.utt_off = torch.from_numpy(offs.astype(np.int32)).to(dev)
        self.frame_off = offs


def _args(pl, mp, momentum=0.0, **ptr):
    a = _lib.GriffinLim()
    a.frames, a.n_fft, a.hop, a.n_utt, a.momentum = mp.frames, pl.n_fft, pl.hop, mp.n_utt, float(momentum)
    a.window, a.twiddle, a.frame_utt, a.utt_off = pl.window_d.data_ptr(), pl.twiddle_d.data_ptr(), mp.frame_utt.data_ptr(), mp.utt_off.data_ptr()
    for k, v in ptr.items():
        setattr(a, k, None if v is None else v.data_ptr())
    return a


# one launch each, on caller-owned buffers (the tests surround them with guard zones)
def launch_mel2lin(pl, mel_rows, S):
    _lib.check(_lib.load().fcl_gl_mel2lin_fwd(mel_rows.data_ptr(), None if pl.stats_d is None else pl.stats_d.data_ptr(), pl.pinv_t_d.data_ptr(), S.data_ptr(),
                                              int(mel_rows.shape[0]), pl.A, pl.bins, ops._stream()))


def launch_phase_init(pl, mp, utt_seed, P, u_out=None):
    _lib.check(_lib.load().fcl_gl_phase_init(C.byref(_args(pl, mp, utt_seed=utt_seed, p=P, u_out=u_out)), ops._stream()))


def launch_synth(pl, mp, S, P, fr):
    _lib.check(_lib.load().fcl_gl_synth_fwd(C.byref(_args(pl, mp, s=S, p=P, fr=fr)), ops._stream()))


def launch_ola(pl, mp, fr, y):
    _lib.check(_lib.load().fcl_gl_ola_fwd(C.byref(_args(pl, mp, fr=fr, y=y)), ops._stream()))


def launch_analysis(pl, mp, y, P, c_prev=None, c_out=None, momentum=0.0):
    _lib.check(_lib.load().fcl_gl_analysis_fwd(C.byref(_args(pl, mp, momentum, y=y, p=P, c_prev=c_prev, c_out=c_out)), ops._stream()))


class GriffinLim(Generator):
    """Griffin-Lim on a GriffinLimPlan, with the generators' surface (`synthesize(..., phase0=)` passes the initial phase on)."""

    def samples_of(self, frames):
        """samples of an utterance of `frames` mel frames: hop * (frames - 1)"""
        return self.plan.hop * (int(frames) - 1)

    def check_lens(self, lens, ids=None):
        check_lens(lens, self.plan.n_fft, self.plan.hop, ids)

    def iterate(self, mp, S, P, n_iter=None):
        """n_iter Griffin-Lim iterations from the magnitudes S [frames, F] and the phase P [frames, F] complex64 (updated in place), then the final
        synthesis -> the packed waveform [hop * (frames - utterances)] (three launches per iteration: synthesis, overlap-add, analysis + phase update)."""
        pl, dev = self.plan, self.plan.device
        n_iter = pl.n_iter if n_iter is None else int(n_iter)
        with torch.cuda.device(dev):
            fr = torch.empty(mp.frames, pl.n_fft, device=dev, dtype=torch.float32)
            flat = torch.empty(pl.hop * (mp.frames - mp.n_utt), device=dev, dtype=torch.float32)
            c_prev = torch.zeros(mp.frames, pl.bins, device=dev, dtype=torch.complex64) if pl.momentum != 0.0 else None
            for _ in range(n_iter):
                launch_synth(pl, mp, S, P, fr)
                launch_ola(pl, mp, fr, flat)
                launch_analysis(pl, mp, flat, P, c_prev, None, pl.momentum)
            launch_synth(pl, mp, S, P, fr)
            launch_ola(pl, mp, fr, flat)
        return flat

    def synthesize_packed(self, mel_rows, lens, noise=None, seed=0, return_intermediates=False, return_flat=False, phase0=None, n_iter=None, ids=None):
        """The same on utterances already packed row-wise ([sum T', n_mels] device tensor) with their frame counts.  Utterance i draws its initial
        phase from seed + i, so a batch equals its per-utterance runs with the same seeds; phase0 ([sum T', F] complex64) replaces the draw.  `noise`
        is accepted and unused.  return_intermediates: also dict(S, P) (the magnitudes and the last phase).  return_flat: also the one buffer the
        waveforms are slices of (utterances back to back)."""
        pl, dev = self.plan, self.plan.device
        lens = self._packed_lens(mel_rows, lens, ids)
        if sum(lens) * pl.n_fft >= 2 ** 31 - 1:
            raise _lib.FclError("fcl-taco2_amd: more than 2^31 / n_fft frames in one Griffin-Lim batch")
        with torch.cuda.device(dev):
            mp = Maps(lens, dev)
            F, bins = mp.frames, pl.bins
            mel_rows = mel_rows.to(device=dev, dtype=torch.float32).contiguous()
            S = torch.empty(F, bins, device=dev, dtype=torch.float32)
            launch_mel2lin(pl, mel_rows, S)
            if phase0 is not None:
                P = torch.as_tensor(phase0).to(device=dev, dtype=torch.complex64).contiguous().clone()
                if tuple(P.shape) != (F, bins):
                    raise _lib.FclError("fcl-taco2_amd: phase0 must be [%d, %d] complex, got %r" % (F, bins, tuple(P.shape)))
            else:
                P = torch.empty(F, bins, device=dev, dtype=torch.complex64)
                seeds = torch.from_numpy(((int(seed) + np.arange(mp.n_utt, dtype=np.int64)) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)).to(dev)
                launch_phase_init(pl, mp, seeds, P)
            flat = self.iterate(mp, S, P, n_iter)
            so = (mp.frame_off - np.arange(mp.n_utt + 1)) * pl.hop
            outs = [flat[int(so[i]) : int(so[i + 1])] for i in range(mp.n_utt)]
            return self._results(outs, dict(S=S, P=P, lens=lens), flat, return_intermediates, return_flat)


def add_analysis_arguments(g):
    """The analysis flags alone (the feature-extraction driver takes these without the Griffin-Lim ones)"""
    g.add_argument("--fs", type=int, default=DEFAULTS["fs"], help="sampling rate")
    g.add_argument("--n-fft", type=int, default=DEFAULTS["n_fft"])
    g.add_argument("--hop", type=int, default=DEFAULTS["hop"])
    g.add_argument("--win-length", type=int, default=None, help="window length (default: n_fft)")
    g.add_argument("--fmin", type=float, default=DEFAULTS["fmin"])
    g.add_argument("--fmax", type=float, default=DEFAULTS["fmax"])


def add_arguments(ap):
    """The drivers' Griffin-Lim flags; the analysis flags default to the reference's preprocess.py."""
    g = ap.add_argument_group("Griffin-Lim (no vocoder checkpoint)")
    g.add_argument("--mel-stats", default=None, metavar="FILE.npy", help="mel_stats.npy of preprocess.py ([2, n_mels]: mean, std): de-normalises the mels")
    g.add_argument("--mel-basis", default=None, metavar="FILE.npy", help="[n_mels, n_fft / 2 + 1] mel filterbank replacing the built Slaney one")
    g.add_argument("--gl-iters", type=int, default=DEFAULTS["n_iter"], help="Griffin-Lim iterations")
    g.add_argument("--gl-momentum", type=float, default=DEFAULTS["momentum"], help="momentum of the fast Griffin-Lim update (0: the classic form)")
    add_analysis_arguments(g)


def check_arguments(ap, args, checkpoint):
    """--griffin-lim and the checkpoint flag are exclusive and one is required; the configuration is checked by name.  Errors end in ap.error (exit 2)."""
    if bool(args.griffin_lim) == bool(checkpoint):
        ap.error("exactly one of --griffin-lim and the vocoder checkpoint flag is required")
    if args.griffin_lim:
        try:
            check_config(args.n_fft, args.hop, args.n_fft if args.win_length is None else args.win_length, fs=args.fs, fmin=args.fmin, fmax=args.fmax,
                         n_iter=args.gl_iters, momentum=args.gl_momentum)
        except (NotImplementedError, ValueError) as e:
            ap.error(str(e))


def from_args(args, device, n_mels=80):
    """(GriffinLim, sampling rate) of a driver's parsed flags"""
    stats = None if args.mel_stats is None else np.load(args.mel_stats)
    basis = None if args.mel_basis is None else np.load(args.mel_basis)
    plan = GriffinLimPlan(device, fs=args.fs, n_fft=args.n_fft, hop=args.hop, win_length=args.win_length, n_mels=n_mels, fmin=args.fmin, fmax=args.fmax,
                          n_iter=args.gl_iters, momentum=args.gl_momentum, mel_stats=stats, mel_basis=basis)
    return GriffinLim(plan), plan.fs
