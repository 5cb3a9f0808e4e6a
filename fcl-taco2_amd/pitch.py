"""YIN F0 tracking on the HIP path: waveform -> frame-level F0 in Hz on the mel features' frame grid (csrc/pitch.hip).

What the feature extraction (features.py) lacked to make every training input from wavs alone: the reference takes its F0 from a third-party
tracker (preprocess.py lines 64-66) that is not available here.  This is YIN (de Cheveigne & Kawahara 2002) steps 1 - 5: difference function over
N / 2 samples, cumulative-mean normalisation, the first dip below the threshold followed downhill, a parabola, then the removal of voiced runs shorter
than min_voiced frames.  The contract is stated in include/fcl_hip.h "F0 tracking" and restated in float64 numpy in tests/pitch_ref.py; parity with
the third-party tracker stays unpinned (DESIGN §6f names the rules a comparison would have to confirm).

method="pyin" (--f0-method pyin; csrc/pyin.hip) keeps the difference function and replaces the single-threshold pick: a Beta(2, 18)
distribution over 100 thresholds gives each frame several period candidates with a probability each (Mauch & Dixon 2014), and a Viterbi pass over a
pitch-and-voicing HMM picks the track -- no octave jump when an even harmonic swells, no voicing that flickers in noise.  Restated in numpy in
tests/pyin_ref.py.

An utterance of L samples gives T = L // hop + 1 frames, the frames of its mel rows, and needs L >= frame_length / 2 + 1.  No CPU fallback."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib, features, griffinlim, ops

# the third-party tracker's F0 range; YIN's threshold; frames, not seconds
DEFAULTS = dict(fs=griffinlim.DEFAULTS["fs"], hop=griffinlim.DEFAULTS["hop"], frame_length=1024, f0_floor=71.0, f0_ceil=800.0, threshold=0.1, min_voiced=3)
FRAME_LENGTHS = (512, 1024)
METHODS = ("yin", "pyin")
# pYIN's published values, untuned: pitch bins per semitone, the fastest pitch change in octaves per second (the band's half width), the Beta(2, 18)
# threshold distribution over 100 thresholds, the share PA of the mass of thresholds below every dip that goes to the global minimum
PYIN_DEFAULTS = dict(bins_per_semitone=5, max_rate=35.92)
PYIN_THRESHOLDS, PYIN_MAX_BINS, PYIN_MAX_BAND, PYIN_SWITCH = 100, 512, 63, 0.01


def tau_range(fs, f0_floor, f0_ceil):
    """(tau_min, tau_max) = (floor(fs / f0_ceil), ceil(fs / f0_floor))"""
    return int(math.floor(fs / f0_ceil)), int(math.ceil(fs / f0_floor))


def pyin_bins(f0_floor, f0_ceil, bins_per_semitone):
    """nb = floor(12 B log2(f0_ceil / f0_floor)) + 1"""
    return int(math.floor(12.0 * bins_per_semitone * math.log2(f0_ceil / f0_floor))) + 1


def pyin_band(fs, hop, bins_per_semitone, max_rate):
    """W = round(max_rate 12 B hop / fs): the bins a track may move per frame"""
    return int(np.round(max_rate * 12.0 * bins_per_semitone * hop / fs))


def pyin_tables(fs, hop, f0_floor, f0_ceil, bins_per_semitone, max_rate):
    """The device tables of csrc/pyin.hip in float64 (include/fcl_hip.h "Probabilistic YIN"): thr, cw, f_bin, edge, tri, la"""
    n, steps = PYIN_THRESHOLDS, 12.0 * bins_per_semitone
    nb, W = pyin_bins(f0_floor, f0_ceil, bins_per_semitone), pyin_band(fs, hop, bins_per_semitone, max_rate)
    i = np.arange(1, n + 1, dtype=np.float64)
    cdf = lambda x: 1.0 - (1.0 - x) ** 18 * (1.0 + 18.0 * x)  # Beta(2, 18)
    k = np.arange(2 * W + 1, dtype=np.float64)
    stay = 1.0 - PYIN_SWITCH
    return dict(thr=i / n, cw=np.concatenate([[0.0], np.cumsum(cdf(i / n) - cdf((i - 1.0) / n))]), f_bin=f0_floor * 2.0 ** (np.arange(nb) / steps),
                edge=fs / (f0_floor * 2.0 ** ((np.arange(nb - 1) + 0.5) / steps)), tri=np.log((W + 1.0 - np.abs(k - W)) / (W + 1.0) ** 2),
                la=np.log(np.array([[stay, PYIN_SWITCH], [PYIN_SWITCH, stay]])))


def check_config(fs, hop, frame_length, f0_floor, f0_ceil, threshold, min_voiced, method="yin", bins_per_semitone=PYIN_DEFAULTS["bins_per_semitone"],
                 max_rate=PYIN_DEFAULTS["max_rate"]):
    """What the kernels cover; anything else is refused naming the flag (NotImplementedError / ValueError) before the first device call."""
    if method not in METHODS:
        raise ValueError("fcl-taco2_amd: pitch: --f0-method %r is not one of %r" % (method, METHODS))
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
    if method == "pyin":
        if not (bins_per_semitone >= 1 and int(bins_per_semitone) == bins_per_semitone):
            raise ValueError("fcl-taco2_amd: pitch: --f0-bins-per-semitone must be a whole number >= 1 (got %r)" % (bins_per_semitone,))
        nb = pyin_bins(f0_floor, f0_ceil, bins_per_semitone)
        if nb > PYIN_MAX_BINS:
            raise ValueError("fcl-taco2_amd: pitch: --f0-bins-per-semitone %d gives %d pitch bins between --f0-floor %g Hz and --f0-ceil %g Hz; the HIP path "
                             "holds at most %d" % (bins_per_semitone, nb, f0_floor, f0_ceil, PYIN_MAX_BINS))
        if not max_rate > 0:
            raise ValueError("fcl-taco2_amd: pitch: --f0-max-rate must be positive (got %r)" % (max_rate,))
        W = pyin_band(fs, hop, bins_per_semitone, max_rate)
        if not 1 <= W <= PYIN_MAX_BAND:
            raise ValueError("fcl-taco2_amd: pitch: --f0-max-rate %g octaves per second is %d pitch bins per frame at --f0-bins-per-semitone %d, --hop %d "
                             "and --fs %d; the HIP path covers 1 .. %d" % (max_rate, W, bins_per_semitone, hop, fs, PYIN_MAX_BAND))


class PitchPlan(object):
    """Configuration of the tracker.  The YIN kernels sum the difference function directly, so method "yin" has no device table: the plan only
    names the device (a GPU: no CPU fallback) and holds the checked numbers.  method "pyin" adds the tables of csrc/pyin.hip, built in float64 and
    uploaded as float32 (tables: the host copies, float32)."""

    def __init__(self, device, fs=DEFAULTS["fs"], hop=DEFAULTS["hop"], frame_length=DEFAULTS["frame_length"], f0_floor=DEFAULTS["f0_floor"],
                 f0_ceil=DEFAULTS["f0_ceil"], threshold=DEFAULTS["threshold"], min_voiced=DEFAULTS["min_voiced"], method="yin",
                 bins_per_semitone=PYIN_DEFAULTS["bins_per_semitone"], max_rate=PYIN_DEFAULTS["max_rate"]):
        check_config(fs, hop, frame_length, f0_floor, f0_ceil, threshold, min_voiced, method, bins_per_semitone, max_rate)
        self.method, self.bins_per_semitone, self.max_rate = method, int(bins_per_semitone), float(max_rate)
        self.fs, self.hop, self.frame_length = int(fs), int(hop), int(frame_length)
        self.f0_floor, self.f0_ceil, self.threshold, self.min_voiced = float(f0_floor), float(f0_ceil), float(threshold), int(min_voiced)
        self.tau_min, self.tau_max = tau_range(self.fs, self.f0_floor, self.f0_ceil)
        self.n_lag = self.tau_max + 2  # d'(0 .. tau_max + 1): the columns of cmnd_out
        if not str(device).startswith("cuda"):
            raise _lib.FclError("fcl-taco2_amd: PitchPlan needs a GPU device (no CPU fallback)")
        self.device = torch.device(device)
        if method == "pyin":
            self.nb, self.band = pyin_bins(self.f0_floor, self.f0_ceil, self.bins_per_semitone), pyin_band(self.fs, self.hop, self.bins_per_semitone, self.max_rate)
            self.tables = {k: v.astype(np.float32) for k, v in pyin_tables(self.fs, self.hop, self.f0_floor, self.f0_ceil, self.bins_per_semitone,
                                                                            self.max_rate).items()}
            # (one bin has no edge: a word of padding keeps the pointer non-null, the kernel reads nb - 1 = 0 of them)
            self.dev_tables = {k: torch.from_numpy(np.ascontiguousarray(v if v.size else np.zeros(1, np.float32)).reshape(-1)).to(self.device)
                               for k, v in self.tables.items()}

    def workspace_bytes(self, frames):
        """what launch_pyin_viterbi needs for a batch of that many frames: one back-pointer byte per frame and state"""
        return int(frames) * 2 * self.nb


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


def _pyin_args(pl, mp):
    a = _lib.Pyin()
    a.frames, a.n_utt, a.n_lag, a.tau_min, a.tau_max, a.nb, a.w, a.fs = mp.frames, mp.n_utt, pl.n_lag, pl.tau_min, pl.tau_max, pl.nb, pl.band, float(pl.fs)
    for k, t in pl.dev_tables.items():
        setattr(a, k, t.data_ptr())
    a.utt_off = mp.utt_off.data_ptr()
    return a


def launch_pyin_obs(pl, mp, cmnd, lv, lu, bf0, ov_out=None):
    """cmnd [frames, tau_max + 2] (launch_yin's cmnd_out) -> lv [frames, nb] and lu [frames], the voiced and unvoiced log-observations, and bf0
    [frames, nb], each bin's F0 (0 where no candidate fell); ov_out [frames, nb], the probability mass per bin, when given"""
    a = _pyin_args(pl, mp)
    a.cmnd, a.lv, a.lu, a.bf0 = cmnd.data_ptr(), lv.data_ptr(), lu.data_ptr(), bf0.data_ptr()
    a.ov_out = None if ov_out is None else ov_out.data_ptr()
    _lib.check(_lib.load().fcl_px_pyin_obs_fwd(C.byref(a), ops._stream()))


def launch_pyin_viterbi(pl, mp, lv, lu, bf0, workspace, state, f0, score):
    """lv, lu, bf0 of launch_pyin_obs -> state [frames] int32 (voiced bin b: b, unvoiced: nb + b), f0 [frames] Hz before the short-run removal and
    score [n_utt]; workspace: uint8, at least pl.workspace_bytes(frames)"""
    a = _pyin_args(pl, mp)
    a.lv, a.lu, a.bf0 = lv.data_ptr(), lu.data_ptr(), bf0.data_ptr()
    a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    a.state, a.f0, a.score = state.data_ptr(), f0.data_ptr(), score.data_ptr()
    _lib.check(_lib.load().fcl_px_pyin_viterbi_fwd(C.byref(a), ops._stream()))


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
        the same batch (same lens and hop), so that one batch's maps serve the mel launch and these.  Under method "pyin" FOUR launches (YIN for d',
        the observations, Viterbi, the short-run removal), and return_cmnd gives the decoded states [sum T] in place of the picked lags."""
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
            if pl.method == "pyin":
                return self._track_pyin(x, mp, return_cmnd)
            raw = torch.empty(mp.frames, device=dev, dtype=torch.float32)
            f0 = torch.empty(mp.frames, device=dev, dtype=torch.float32)
            cm = torch.empty(mp.frames, pl.n_lag, device=dev, dtype=torch.float32) if return_cmnd else None
            tau = torch.empty(mp.frames, device=dev, dtype=torch.int32) if return_cmnd else None
            launch_yin(pl, mp, x, raw, cm, tau)
            launch_short_run(mp, raw, f0, pl.min_voiced)
        return (f0, mp.lens, cm, tau) if return_cmnd else (f0, mp.lens)

    def _track_pyin(self, x, mp, return_cmnd):
        pl, dev = self.plan, self.plan.device
        if mp.frames * 2 * pl.nb >= 2 ** 31 - 1:
            raise _lib.FclError("fcl-taco2_amd: more than 2^31 frames x states in one pitch batch")
        new = lambda *shape, **kw: torch.empty(*shape, device=dev, dtype=kw.get("dtype", torch.float32))
        yin, raw, f0, cm = new(mp.frames), new(mp.frames), new(mp.frames), new(mp.frames, pl.n_lag)
        lv, lu, bf0 = new(mp.frames, pl.nb), new(mp.frames), new(mp.frames, pl.nb)
        state, score, ws = new(mp.frames, dtype=torch.int32), new(mp.n_utt), new(pl.workspace_bytes(mp.frames), dtype=torch.uint8)
        launch_yin(pl, mp, x, yin, cm)  # its own pick (yin) is not used: d' is what goes on
        launch_pyin_obs(pl, mp, cm, lv, lu, bf0)
        launch_pyin_viterbi(pl, mp, lv, lu, bf0, ws, state, raw, score)
        launch_short_run(mp, raw, f0, pl.min_voiced)
        return (f0, mp.lens, cm, state) if return_cmnd else (f0, mp.lens)

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
    g.add_argument("--f0-threshold", type=float, default=DEFAULTS["threshold"],
                   help="YIN's threshold on the normalised difference function (ignored under --f0-method pyin, which weighs 100 thresholds)")
    g.add_argument("--f0-min-voiced", type=int, default=DEFAULTS["min_voiced"], metavar="FRAMES", help="voiced runs shorter than this become unvoiced (1: keep all)")
    g.add_argument("--f0-frame-length", type=int, default=DEFAULTS["frame_length"], metavar="N", help="pitch frame length (512 or 1024); half of it is integrated over")


    g.add_argument("--f0-method", choices=METHODS, default="yin",
                   help="yin: every frame alone, the first dip below --f0-threshold; pyin: probabilistic YIN, several candidates per frame and a Viterbi "
                        "pass over pitch and voicing (steadier against octave jumps and noise)")
    g.add_argument("--f0-bins-per-semitone", type=int, default=PYIN_DEFAULTS["bins_per_semitone"], metavar="B",
                   help="pyin: resolution of the pitch states (at most 512 bins between --f0-floor and --f0-ceil)")
    g.add_argument("--f0-max-rate", type=float, default=PYIN_DEFAULTS["max_rate"], metavar="OCT_PER_S",
                   help="pyin: the fastest pitch change a track may make, in octaves per second (1 .. 63 bins per frame)")


def check_arguments(ap, args):
    """the configuration is checked naming the flag; errors end in ap.error (exit 2)"""
    try:
        check_config(args.fs, args.hop, args.f0_frame_length, args.f0_floor, args.f0_ceil, args.f0_threshold, args.f0_min_voiced, args.f0_method,
                     args.f0_bins_per_semitone, args.f0_max_rate)
    except (NotImplementedError, ValueError) as e:
        ap.error(str(e))


def from_args(args, device):
    """PitchTracker of a driver's parsed flags (add_pitch_arguments and griffinlim.add_analysis_arguments)"""
    return PitchTracker(PitchPlan(device, fs=args.fs, hop=args.hop, frame_length=args.f0_frame_length, f0_floor=args.f0_floor, f0_ceil=args.f0_ceil,
                                  threshold=args.f0_threshold, min_voiced=args.f0_min_voiced, method=args.f0_method,
                                  bins_per_semitone=args.f0_bins_per_semitone, max_rate=args.f0_max_rate))
