"""YIN F0 tracking on the HIP path: waveform -> frame-level F0 in Hz on the mel features' frame grid (csrc/pitch.hip).

What the feature extraction (features.py) lacked to make every training input from wavs alone: the reference takes its F0 from a third-party
tracker (preprocess.py lines 64-66) that is not available here.  This is YIN (de Cheveigne & Kawahara 2002) steps 1 - 5: difference function over
N / 2 samples, cumulative-mean normalisation, the first dip below the threshold followed downhill, a parabola, then the removal of voiced runs shorter
than min_voiced frames.  The contract is stated in include/fcl_hip.h "F0 tracking" and restated in float64 numpy in tests/pitch_ref.py; parity with
the third-party tracker stays unpinned (DESIGN §6f names the rules a comparison would have to confirm).

An utterance of L samples gives T = L // hop + 1 frames, the frames of its mel rows, and needs L >= frame_length / 2 + 1.  No CPU fallback."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib, features, griffinlim, ops

# the third-party tracker's F0 range; YIN's threshold; frames, not seconds
DEFAULTS = dict(fs=griffinlim.DEFAULTS["fs"], hop=griffinlim.DEFAULTS["hop"], frame_length=1024, f0_floor=71.0, f0_ceil=800.0, threshold=0.1, min_voiced=3)
FRAME_LENGTHS = (512, 1024)


def tau_range(fs, f0_floor, f0_ceil):
    """(tau_min, tau_max) = (floor(fs / f0_ceil), ceil(fs / f0_floor))"""
    return int(math.floor(fs / f0_ceil)), int(math.ceil(fs / f0_floor))


def check_config(fs, hop, frame_length, f0_floor, f0_ceil, threshold, min_voiced):
    """What the kernels cover; anything else is refused naming the flag (NotImplementedError / ValueError) before the first device call."""
    if frame_length not in FRAME_LENGTHS:
        raise NotImplementedError("fcl-taco2_amd: pitch: --f0-frame-length %r is not supported on the HIP path (one of %r)" % (frame_length, FRAME_LENGTHS))
    if hop < 1:
        raise NotImplementedError("fcl-taco2_amd: pitch: --hop %r is not supported (hop >= 1)" % (hop,))
    if not (fs > 0 and f0_floor > 0 and f0_ceil > 0):
        raise ValueError("fcl-taco2_amd: pitch: --fs, --f0-floor and --f0-ceil must be positive (got %r, %r, %r)" % (fs, f0_floor, f0_ceil))
    tau_min, tau_max = tau_range(fs, f0_floor, f0_ceil)
    if tau_min < 2:
        raise ValueError("fcl-taco2_amd: pitch: --f0-ceil %g Hz is too high for --fs %d: the shortest lag floor(fs / f0_ceil) = %d must be at least 2"
                         % (f0_ceil, fs, tau_min))
    if tau_max > frame_length // 2 - 1:
        raise ValueError("fcl-taco2_amd: pitch: --f0-floor %g Hz is too low for --f0-frame-length %d at --fs %d: the longest lag ceil(fs / f0_floor) = %d "
                         "must not exceed frame_length / 2 - 1 = %d" % (f0_floor, frame_length, fs, tau_max, frame_length // 2 - 1))
    if tau_min >= tau_max:
        raise ValueError("fcl-taco2_amd: pitch: --f0-floor %g Hz must lie below --f0-ceil %g Hz by at least one lag (lags %d .. %d)"
                         % (f0_floor, f0_ceil, tau_min, tau_max))
    if not 0.0 < threshold <= 1.0:
        raise ValueError("fcl-taco2_amd: pitch: --f0-threshold must lie in (0, 1] (got %r)" % (threshold,))
    if min_voiced < 1:
        raise ValueError("fcl-taco2_amd: pitch: --f0-min-voiced must be at least 1 (got %r)" % (min_voiced,))


class PitchPlan(object):
    """Configuration of the tracker.  The kernels sum the difference function directly, so there is no device table: the plan only names the
    device (a GPU: no CPU fallback) and holds the checked numbers."""

    def __init__(self, device, fs=DEFAULTS["fs"], hop=DEFAULTS["hop"], frame_length=DEFAULTS["frame_length"], f0_floor=DEFAULTS["f0_floor"],
                 f0_ceil=DEFAULTS["f0_ceil"], threshold=DEFAULTS["threshold"], min_voiced=DEFAULTS["min_voiced"]):
        check_config(fs, hop, frame_length, f0_floor, f0_ceil, threshold, min_voiced)
        self.fs, self.hop, self.frame_length = int(fs), int(hop), int(frame_length)
        self.f0_floor, self.f0_ceil, self.threshold, self.min_voiced = float(f0_floor), float(f0_ceil), float(threshold), int(min_voiced)
        self.tau_min, self.tau_max = tau_range(self.fs, self.f0_floor, self.f0_ceil)
        self.n_lag = self.tau_max + 2  # d'(0 .. tau_max + 1): the columns of cmnd_out
        if not str(device).startswith("cuda"):
            raise _lib.FclError("fcl-taco2_amd: PitchPlan needs a GPU device (no CPU fallback)")
        self.device = torch.device(device)


# one launch each, on caller-owned buffers (the tests surround them with guard zones)
def launch_yin(pl, mp, x, f0, cmnd_out=None, tau_out=None):
    """x [samples] float32 -> f0 [frames] float32 Hz (0 = unvoiced), before the short-run removal; cmnd_out [frames, tau_max + 2] float32 and
    tau_out [frames] int32 when given"""
    a = _lib.Pitch()
    a.frames, a.samples, a.n, a.hop, a.n_utt, a.tau_min, a.tau_max = mp.frames, mp.samples, pl.frame_length, pl.hop, mp.n_utt, pl.tau_min, pl.tau_max
    a.fs, a.threshold = float(pl.fs), pl.threshold
    a.x, a.smp_off, a.frame_utt, a.utt_off = x.data_ptr(), mp.smp_off.data_ptr(), mp.frame_utt.data_ptr(), mp.utt_off.data_ptr()
    a.f0 = f0.data_ptr()
    a.cmnd_out, a.tau_out = None if cmnd_out is None else cmnd_out.data_ptr(), None if tau_out is None else tau_out.data_ptr()
    _lib.check(_lib.load().fcl_px_yin_fwd(C.byref(a), ops._stream()))


def launch_short_run(mp, f0_in, f0_out, min_voiced):
    """f0_in [frames] -> f0_out [frames] (another buffer): voiced runs shorter than min_voiced frames inside one utterance become 0"""
    _lib.check(_lib.load().fcl_px_short_run_fwd(f0_in.data_ptr(), mp.frame_utt.data_ptr(), mp.utt_off.data_ptr(), f0_out.data_ptr(), mp.frames, mp.n_utt,
                                                int(min_voiced), ops._stream()))


class PitchTracker(object):
    """F0 tracking on a PitchPlan."""

    def __init__(self, plan):
        self.plan = plan

    def frames_of(self, n_samples):
        return features.frames_of(n_samples, self.plan.hop)

    def check_lens(self, lens, ids=None):
        """every utterance needs frame_length / 2 + 1 samples; the first shorter one is refused by id"""
        need = features.min_samples(self.plan.frame_length)
        for i, n in enumerate(lens):
            if int(n) < need:
                raise ValueError("fcl-taco2_amd: pitch: utterance %s has %d samples; --f0-frame-length %d needs at least %d (frame_length / 2 + 1: a single "
                                 "reflection at either end)" % (ids[i] if ids is not None else "#%d" % i, int(n), self.plan.frame_length, need))

    def track_packed(self, wave, lens, ids=None, return_cmnd=False, maps=None):
        """wave: the utterances' samples back to back ([sum L] float32, device tensor or array), lens: samples per utterance -> (f0 [sum T] Hz with
        0 = unvoiced, frame_lens) (+ d' [sum T, tau_max + 2] and the picked lags [sum T] with return_cmnd): TWO launches.  maps: the features.Maps of
        the same batch (same lens and hop), so that one batch's maps serve the mel launch and these."""
        pl, dev = self.plan, self.plan.device
        lens = [int(n) for n in lens]
        self.check_lens(lens, ids)
        with torch.cuda.device(dev):
            x = torch.as_tensor(wave).to(device=dev, dtype=torch.float32).contiguous().reshape(-1)
            if x.numel() != sum(lens):
                raise _lib.FclError("fcl-taco2_amd: pitch: the packed waveform has %d samples, lens sum to %d" % (x.numel(), sum(lens)))
            mp = features.Maps(lens, pl.hop, dev) if maps is None else maps
            if mp.sample_lens != lens:
                raise _lib.FclError("fcl-taco2_amd: pitch: the maps passed in belong to another batch")
            if mp.samples >= 2 ** 31 - 1 or mp.frames * pl.n_lag >= 2 ** 31 - 1:
                raise _lib.FclError("fcl-taco2_amd: more than 2^31 samples or frames x lags in one pitch batch")
            raw = torch.empty(mp.frames, device=dev, dtype=torch.float32)
            f0 = torch.empty(mp.frames, device=dev, dtype=torch.float32)
            cm = torch.empty(mp.frames, pl.n_lag, device=dev, dtype=torch.float32) if return_cmnd else None
            tau = torch.empty(mp.frames, device=dev, dtype=torch.int32) if return_cmnd else None
            launch_yin(pl, mp, x, raw, cm, tau)
            launch_short_run(mp, raw, f0, pl.min_voiced)
        return (f0, mp.lens, cm, tau) if return_cmnd else (f0, mp.lens)

    def track(self, waves, ids=None):
        """list of 1-D float arrays -> list of F0 tracks [T] (device tensors).  A waveform whose peak exceeds 1 is divided by its peak, as
        FeatureExtractor.extract does (the tracker itself is invariant to scale; the division keeps both on the same samples)."""
        xs = []
        for w in waves:
            w = np.asarray(w, dtype=np.float32).reshape(-1)
            peak = float(np.abs(w).max()) if len(w) else 0.0
            xs.append(w / np.float32(peak) if peak > 1.0 else w)
        f0, frame_lens = self.track_packed(np.concatenate(xs), [len(w) for w in xs], ids=ids)
        offs = np.concatenate([[0], np.cumsum(frame_lens)])
        return [f0[offs[i] : offs[i + 1]] for i in range(len(xs))]


def add_pitch_arguments(g):
    """The drivers' F0 flags (--fs and --hop come with the analysis flags)"""
    g.add_argument("--f0-floor", type=float, default=DEFAULTS["f0_floor"], metavar="HZ", help="lowest F0 looked for: the longest lag is ceil(fs / f0_floor)")
    g.add_argument("--f0-ceil", type=float, default=DEFAULTS["f0_ceil"], metavar="HZ", help="highest F0 looked for: the shortest lag is floor(fs / f0_ceil)")
    g.add_argument("--f0-threshold", type=float, default=DEFAULTS["threshold"], help="YIN's threshold on the normalised difference function")
    g.add_argument("--f0-min-voiced", type=int, default=DEFAULTS["min_voiced"], metavar="FRAMES", help="voiced runs shorter than this become unvoiced (1: keep all)")
    g.add_argument("--f0-frame-length", type=int, default=DEFAULTS["frame_length"], metavar="N", help="pitch frame length (512 or 1024); half of it is integrated over")


def check_arguments(ap, args):
    """the configuration is checked naming the flag; errors end in ap.error (exit 2)"""
    try:
        check_config(args.fs, args.hop, args.f0_frame_length, args.f0_floor, args.f0_ceil, args.f0_threshold, args.f0_min_voiced)
    except (NotImplementedError, ValueError) as e:
        ap.error(str(e))


def from_args(args, device):
    """PitchTracker of a driver's parsed flags (add_pitch_arguments and griffinlim.add_analysis_arguments)"""
    return PitchTracker(PitchPlan(device, fs=args.fs, hop=args.hop, frame_length=args.f0_frame_length, f0_floor=args.f0_floor, f0_ceil=args.f0_ceil,
                                  threshold=args.f0_threshold, min_voiced=args.f0_min_voiced))
