"""Log-mel and energy feature extraction on the HIP path: waveform -> the training inputs (csrc/features.hip).

The forward half of griffinlim.py, with the same constants (preprocess.py lines 40-50, 71: log10 mel of an STFT magnitude, n_fft 1024, hop 256,
periodic Hann, 80 Slaney mels over 80 - 7600 Hz at 22.05 kHz): reflect-padded centred frames, real FFT, |X|, the mel projection with the floor
1e-10 and log10, the frame energy ||S||_2, and phoneme-level means over the frames a duration vector assigns.  The contract is stated in
include/fcl_hip.h and restated in float64 numpy in tests/features_ref.py; the third-party analysis code of the reference's preprocessing is not
available here, so parity with it stays unpinned (DESIGN §6e names the rules a comparison would have to confirm).

An utterance of L samples gives T = L // hop + 1 frames and needs L >= n_fft / 2 + 1.  No CPU fallback."""
import ctypes as C

import numpy as np
import torch

from . import _lib, griffinlim, ops

DEFAULTS = {k: griffinlim.DEFAULTS[k] for k in ("fs", "n_fft", "hop", "win_length", "n_mels", "fmin", "fmax")}


def banded_filterbank(B):
    """B [n_mels, F] -> (fb_lo [n_mels], fb_off [n_mels + 1], fb_w [nnz]): each row's run from its first to its last non-zero bin (an all-zero row:
    an empty run at bin 0).  A row with a zero inside that run is no contiguous band and is refused by name."""
    B = np.asarray(B, dtype=np.float64)
    lo, off, w = [], [0], []
    for c, row in enumerate(B):
        nz = np.flatnonzero(row)
        if len(nz) == 0:
            lo.append(0)
            off.append(off[-1])
            continue
        a, b = int(nz[0]), int(nz[-1]) + 1
        if len(nz) != b - a:
            raise ValueError("fcl-taco2_amd: features: mel_basis row %d is not a contiguous band (non-zero bins %d .. %d with %d zeros between them)"
                             % (c, a, b - 1, b - a - len(nz)))
        lo.append(a)
        off.append(off[-1] + b - a)
        w.append(row[a:b])
    w = np.concatenate(w) if w else np.zeros(0)
    if len(w) == 0:
        raise ValueError("fcl-taco2_amd: features: mel_basis is all zero")
    return np.asarray(lo, dtype=np.int32), np.asarray(off, dtype=np.int32), w


def dense_filterbank(fb_lo, fb_off, fb_w, bins):
    """the inverse of banded_filterbank"""
    B = np.zeros((len(fb_lo), bins), dtype=np.asarray(fb_w).dtype)
    for c, a in enumerate(fb_lo):
        n = int(fb_off[c + 1] - fb_off[c])
        B[c, a : a + n] = fb_w[fb_off[c] : fb_off[c + 1]]
    return B


def frames_of(n_samples, hop):
    """frames of an utterance of n_samples samples: n_samples // hop + 1"""
    return int(n_samples) // int(hop) + 1


def min_samples(n_fft):
    """the shortest utterance: n_fft / 2 + 1 samples, so that the reflection at either end is a single one"""
    return int(n_fft) // 2 + 1


def check_lens(lens, n_fft, ids=None):
    """Every utterance needs min_samples(n_fft) samples; the first shorter one is refused by id (its position without ids)."""
    need = min_samples(n_fft)
    for i, n in enumerate(lens):
        if int(n) < need:
            raise ValueError("fcl-taco2_amd: features: utterance %s has %d samples; n_fft %d needs at least %d (n_fft / 2 + 1: a single reflection at "
                             "either end)" % (ids[i] if ids is not None else "#%d" % i, int(n), n_fft, need))


def adjust_durations(durations, frame_lens, ids=None):
    """Per utterance: the last duration grows (or shrinks) by T - sum(durations), so that the phonemes cover the T frames exactly.  A last duration
    that would turn negative is refused, naming the utterance.  -> list of int64 arrays."""
    out = []
    for i, (d, T) in enumerate(zip(durations, frame_lens)):
        d = np.array(d, dtype=np.int64).reshape(-1)
        name = ids[i] if ids is not None else "#%d" % i
        if len(d) == 0 or (d < 0).any():
            raise ValueError("fcl-taco2_amd: features: utterance %s needs at least one duration and none negative" % name)
        d[-1] += int(T) - int(d.sum())
        if d[-1] < 0:
            raise ValueError("fcl-taco2_amd: features: utterance %s has %d frames but its durations without the last sum to %d: the adjusted last "
                             "duration would be %d" % (name, int(T), int(d[:-1].sum()), int(d[-1])))
        out.append(d)
    return out


class FeaturePlan(object):
    """Configuration and device tables: the banded mel filterbank (built in float64, uploaded as float32), window, twiddles.  `mel_basis`
    ([n_mels, F] array) replaces the built filterbank; `mel_stats` ([2, n_mels]: mean, std) normalises the output."""

    def __init__(self, device, fs=DEFAULTS["fs"], n_fft=DEFAULTS["n_fft"], hop=DEFAULTS["hop"], win_length=DEFAULTS["win_length"], n_mels=DEFAULTS["n_mels"],
                 fmin=DEFAULTS["fmin"], fmax=DEFAULTS["fmax"], mel_stats=None, mel_basis=None):
        win_length = int(n_fft if win_length is None else win_length)
        if mel_basis is not None:
            mel_basis = np.asarray(mel_basis, dtype=np.float64)
            if mel_basis.ndim != 2:
                raise ValueError("fcl-taco2_amd: features: mel_basis must be a [n_mels, n_fft / 2 + 1] matrix, got shape %r" % (mel_basis.shape,))
            n_mels = int(mel_basis.shape[0])
        griffinlim.check_config(n_fft, hop, win_length, n_mels, fs, fmin, fmax)
        self.fs, self.n_fft, self.hop, self.win_length, self.A = int(fs), int(n_fft), int(hop), win_length, int(n_mels)
        self.fmin, self.fmax, self.bins = float(fmin), float(fmax), int(n_fft) // 2 + 1
        if mel_basis is not None and mel_basis.shape[1] != self.bins:
            raise ValueError("fcl-taco2_amd: features: mel_basis has %d columns, n_fft %d needs %d" % (mel_basis.shape[1], self.n_fft, self.bins))
        if mel_stats is not None:
            mel_stats = np.asarray(mel_stats, dtype=np.float64)
            if mel_stats.shape != (2, self.A):
                raise ValueError("fcl-taco2_amd: features: mel_stats must be [2, %d] (mean, std), got %r" % (self.A, mel_stats.shape))
        self.B = griffinlim.mel_filterbank(self.fs, self.n_fft, self.A, self.fmin, self.fmax) if mel_basis is None else mel_basis
        self.fb_lo, self.fb_off, self.fb_w = banded_filterbank(self.B)
        self.nnz = int(len(self.fb_w))
        self.window = griffinlim.hann_window(self.win_length, self.n_fft)
        self.mel_stats = mel_stats
        if not str(device).startswith("cuda"):
            raise _lib.FclError("fcl-taco2_amd: FeaturePlan needs a GPU device (no CPU fallback)")
        self.device = dev = torch.device(device)
        t = lambda a, dt=np.float32: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
        with torch.cuda.device(dev):
            self.window_d, self.twiddle_d = t(self.window), t(griffinlim.twiddles(self.n_fft))
            self.fb_lo_d, self.fb_off_d, self.fb_w_d = t(self.fb_lo, np.int32), t(self.fb_off, np.int32), t(self.fb_w)
            self.stats_d = None if mel_stats is None else t(mel_stats)


class Maps(griffinlim.Maps):
    """frame_utt / utt_off of a batch from its SAMPLE counts, plus smp_off [n_utt + 1] on the device"""

    def __init__(self, sample_lens, hop, dev):
        self.sample_lens = [int(n) for n in sample_lens]
        griffinlim.Maps.__init__(self, [frames_of(n, hop) for n in self.sample_lens], dev)
        self.samples = sum(self.sample_lens)
        self.smp_off = torch.from_numpy(np.concatenate([[0], np.cumsum(self.sample_lens)]).astype(np.int32)).to(dev)


# one launch each, on caller-owned buffers (the tests surround them with guard zones)
def launch_logmel(pl, mp, x, mel, energy, mag_out=None, stats=True):
    """x [samples] float32 -> mel [frames, n_mels], energy [frames] (and mag_out [frames, F]); stats=False leaves the plan's mel_stats out"""
    a = _lib.Features()
    a.frames, a.samples, a.n_fft, a.hop, a.n_utt, a.n_mels, a.nnz = mp.frames, mp.samples, pl.n_fft, pl.hop, mp.n_utt, pl.A, pl.nnz
    a.x, a.smp_off, a.frame_utt, a.utt_off = x.data_ptr(), mp.smp_off.data_ptr(), mp.frame_utt.data_ptr(), mp.utt_off.data_ptr()
    a.window, a.twiddle = pl.window_d.data_ptr(), pl.twiddle_d.data_ptr()
    a.fb_lo, a.fb_off, a.fb_w = pl.fb_lo_d.data_ptr(), pl.fb_off_d.data_ptr(), pl.fb_w_d.data_ptr()
    a.mel_stats = pl.stats_d.data_ptr() if stats and pl.stats_d is not None else None
    a.mel, a.energy, a.mag_out = mel.data_ptr(), energy.data_ptr(), None if mag_out is None else mag_out.data_ptr()
    _lib.check(_lib.load().fcl_fx_logmel_fwd(C.byref(a), ops._stream()))


def launch_segment_mean(v, mask, dur, ph_utt, ph_off, utt_off, out, n_utt, nonzero_only=False):
    """v / mask [frames] float32, dur / ph_utt [n_ph] int32, ph_off / utt_off [n_utt + 1] int32 -> out [n_ph] float32"""
    _lib.check(_lib.load().fcl_fx_segment_mean_fwd(v.data_ptr(), None if mask is None else mask.data_ptr(), dur.data_ptr(), ph_utt.data_ptr(), ph_off.data_ptr(),
                                                   utt_off.data_ptr(), out.data_ptr(), int(dur.numel()), int(n_utt), int(v.numel()), int(bool(nonzero_only)),
                                                   ops._stream()))


class FeatureExtractor(object):
    """Feature extraction on a FeaturePlan."""

    def __init__(self, plan):
        self.plan = plan

    def frames_of(self, n_samples):
        return frames_of(n_samples, self.plan.hop)

    def check_lens(self, lens, ids=None):
        check_lens(lens, self.plan.n_fft, ids)

    def extract_packed(self, wave, lens, return_magnitudes=False, ids=None, maps=None):
        """wave: the utterances' samples back to back ([sum L] float32, device tensor or array), lens: samples per utterance ->
        (mel_rows [sum T, n_mels], energy [sum T], frame_lens) (+ the magnitudes [sum T, F] with return_magnitudes): ONE launch.  maps: the batch's
        Maps when the caller has built them already (pitch.PitchTracker.track_packed takes the same ones)."""
        pl, dev = self.plan, self.plan.device
        lens = [int(n) for n in lens]
        self.check_lens(lens, ids)
        with torch.cuda.device(dev):
            x = torch.as_tensor(wave).to(device=dev, dtype=torch.float32).contiguous().reshape(-1)
            if x.numel() != sum(lens):
                raise _lib.FclError("fcl-taco2_amd: features: the packed waveform has %d samples, lens sum to %d" % (x.numel(), sum(lens)))
            mp = Maps(lens, pl.hop, dev) if maps is None else maps
            if mp.sample_lens != lens:
                raise _lib.FclError("fcl-taco2_amd: features: the maps passed in belong to another batch")
            if mp.samples >= 2 ** 31 - 1 or mp.frames * max(pl.bins, pl.A) >= 2 ** 31 - 1:
                raise _lib.FclError("fcl-taco2_amd: more than 2^31 samples or frames x bins in one feature batch")
            mel = torch.empty(mp.frames, pl.A, device=dev, dtype=torch.float32)
            energy = torch.empty(mp.frames, device=dev, dtype=torch.float32)
            mag = torch.empty(mp.frames, pl.bins, device=dev, dtype=torch.float32) if return_magnitudes else None
            launch_logmel(pl, mp, x, mel, energy, mag)
        return (mel, energy, mp.lens, mag) if return_magnitudes else (mel, energy, mp.lens)

    def extract(self, waves, ids=None):
        """list of 1-D float arrays -> list of (mel [T, n_mels], energy [T]) device tensors.  A waveform whose peak exceeds 1 is divided by its peak."""
        xs = []
        for w in waves:
            w = np.asarray(w, dtype=np.float32).reshape(-1)
            peak = float(np.abs(w).max()) if len(w) else 0.0
            xs.append(w / np.float32(peak) if peak > 1.0 else w)
        mel, energy, frame_lens = self.extract_packed(np.concatenate(xs), [len(w) for w in xs], ids=ids)
        offs = np.concatenate([[0], np.cumsum(frame_lens)])
        return [(mel[offs[i] : offs[i + 1]], energy[offs[i] : offs[i + 1]]) for i in range(len(xs))]

    def phoneme_means(self, values, frame_lens, durations, mask=None, ids=None):
        """values [sum T] (device tensor or array), durations: per utterance an integer vector -> (means [sum P] device tensor, adjusted durations).
        Each utterance's last duration is first increased by T - sum(durations) on the host (adjust_durations).  mask: only frames whose mask
        value is non-zero count (log F0 over voiced frames); a phoneme without such a frame gives 0."""
        dev = self.plan.device
        frame_lens = [int(n) for n in frame_lens]
        durs = adjust_durations(durations, frame_lens, ids)
        n_utt = len(frame_lens)
        if len(durs) != n_utt:
            raise _lib.FclError("fcl-taco2_amd: features: %d duration vectors for %d utterances" % (len(durs), n_utt))
        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
        with torch.cuda.device(dev):
            v = torch.as_tensor(values).to(device=dev, dtype=torch.float32).contiguous().reshape(-1)
            m = None if mask is None else torch.as_tensor(mask).to(device=dev, dtype=torch.float32).contiguous().reshape(-1)
            if v.numel() != sum(frame_lens) or (m is not None and m.numel() != v.numel()):
                raise _lib.FclError("fcl-taco2_amd: features: values / mask must hold sum(frame_lens) = %d entries" % sum(frame_lens))
            n_ph = [len(d) for d in durs]
            out = torch.empty(sum(n_ph), device=dev, dtype=torch.float32)
            launch_segment_mean(v, m, i32(np.concatenate(durs)), i32(np.repeat(np.arange(n_utt), n_ph)), i32(np.concatenate([[0], np.cumsum(n_ph)])),
                                i32(np.concatenate([[0], np.cumsum(frame_lens)])), out, n_utt, m is not None)
        return out, durs


def from_args(args, device, mel_stats=None):
    """FeatureExtractor of a driver's parsed analysis flags (griffinlim.add_arguments)"""
    basis = None if args.mel_basis is None else np.load(args.mel_basis)
    return FeatureExtractor(FeaturePlan(device, fs=args.fs, n_fft=args.n_fft, hop=args.hop, win_length=args.win_length, n_mels=args.n_mels, fmin=args.fmin,
                                        fmax=args.fmax, mel_stats=mel_stats, mel_basis=basis))
