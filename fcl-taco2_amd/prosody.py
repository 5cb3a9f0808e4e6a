"""Prosody control: FastSpeech2-style editing of the predicted speaking rate, pitch and energy before the decoder runs.

A control holds five values per phoneme row -- duration scale a, pitch scale / shift, energy scale / shift -- given per utterance (scalars)
or per phoneme (arrays).  The identity is (1, 1, 0, 1, 0).  The rules (include/fcl_hip.h, fcl_duration_round_ctl_fwd and
fcl_variance_embed_add_ctl_fwd, apply them on the device; `duration_rule` restates the integer one in numpy):

  * duration: d = max(rint(exp(x) - 1), 0) as predicted; if a != 1 and d >= 1: d' = max(rint(fp32(d) * fp32(a)), 1), rint half-to-even.
    A scaled duration is never 0 (the decoder rejects a zero duration); a predicted 0 stays 0 and raises as it does without a control.
  * pitch / energy: p' = fmaf(p, scale, shift), applied only where (scale, shift) != (1, 0), so the identity is exact.  The values live in
    the model's z-normalised domain; `ProsodyControl.from_units` maps semitones / pitch range / energy gain onto the affine with the
    statistics preprocessing writes (f0_en_stats.npy = [f0_mean, f0_std, en_mean, en_std]).

Controls edit the model's PREDICTIONS: forced durations with a != 1, or forced pitch / energy with a non-identity pitch / energy control, are
errors (callers who supply their own values edit them themselves).
"""
import math

import numpy as np

FIELDS = ("duration_scale", "pitch_scale", "pitch_shift", "energy_scale", "energy_shift")
IDENTITY = (1.0, 1.0, 0.0, 1.0, 0.0)
NCTL = len(FIELDS)  # floats per control row (ctl_ld of the C ABI)
DURATION_SCALE_MAX = 8.0


class ProsodyControl(object):
    """Per-utterance (scalar) or per-phoneme (1-D array) values of the five controls."""

    __slots__ = FIELDS

    def __init__(self, duration_scale=1.0, pitch_scale=1.0, pitch_shift=0.0, energy_scale=1.0, energy_shift=0.0):
        for name, v in zip(FIELDS, (duration_scale, pitch_scale, pitch_shift, energy_scale, energy_shift)):
            a = np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, dtype=np.float64)
            if a.ndim > 1:
                raise ValueError("prosody control %s: a scalar or a 1-D per-phoneme array, got shape %s" % (name, a.shape))
            if not np.all(np.isfinite(a)):
                raise ValueError("prosody control %s: every value must be finite" % name)
            if name == "duration_scale" and not np.all((a > 0.0) & (a <= DURATION_SCALE_MAX)):
                raise ValueError("prosody control duration_scale must lie in (0, %g], got %s" % (DURATION_SCALE_MAX, a.min() if a.size else a))
            setattr(self, name, float(a) if a.ndim == 0 else a.astype(np.float32))

    @classmethod
    def from_units(cls, stats=None, semitones=0.0, pitch_range=1.0, energy_gain=1.0, duration_scale=1.0):
        """User units -> the normalised-domain affine.  stats: [f0_mean, f0_std, en_mean, en_std] (f0_en_stats.npy; an array or a path), needed
        for a semitone shift or an energy gain: shift k semitones -> pitch_shift = k ln2 / (12 f0_std); pitch range r -> pitch_scale = r;
        energy gain g -> energy_scale = g, energy_shift = (g - 1) en_mean / en_std."""
        semitones, pitch_range, energy_gain = (np.asarray(v, dtype=np.float64) for v in (semitones, pitch_range, energy_gain))
        need = bool(np.any(semitones != 0.0) or np.any(energy_gain != 1.0))
        if need and stats is None:
            raise ValueError("prosody: a semitone shift or an energy gain needs the feature statistics (f0_en_stats.npy)")
        pitch_shift, energy_shift = 0.0, 0.0
        if need:
            st = np.load(stats) if isinstance(stats, str) else np.asarray(stats, dtype=np.float64)
            st = np.asarray(st, dtype=np.float64).reshape(-1)
            if st.shape[0] != 4 or not np.all(np.isfinite(st)) or st[1] <= 0.0 or st[3] <= 0.0:
                raise ValueError("prosody: stats must be [f0_mean, f0_std, en_mean, en_std] with positive standard deviations")
            f0_std, en_mean, en_std = st[1], st[2], st[3]
            pitch_shift = semitones * math.log(2.0) / (12.0 * f0_std)
            energy_shift = (energy_gain - 1.0) * en_mean / en_std
        return cls(duration_scale=duration_scale, pitch_scale=pitch_range, pitch_shift=pitch_shift, energy_scale=energy_gain,
                   energy_shift=energy_shift)

    @classmethod
    def coerce(cls, obj):
        """None / ProsodyControl / {field: value} -> ProsodyControl or None."""
        if obj is None or isinstance(obj, ProsodyControl):
            return obj
        if isinstance(obj, dict):
            bad = sorted(set(obj) - set(FIELDS))
            if bad:
                raise ValueError("prosody: unknown control field(s) %s (fields: %s)" % (", ".join(bad), ", ".join(FIELDS)))
            return cls(**obj)
        raise TypeError("prosody: expected a ProsodyControl or a dict of %s, got %r" % ("/".join(FIELDS), type(obj).__name__))

    def _is(self, names):
        return all(np.all(np.asarray(getattr(self, n)) == IDENTITY[FIELDS.index(n)]) for n in names)

    @property
    def is_identity(self):
        return self._is(FIELDS)

    @property
    def scales_duration(self):
        return not self._is(FIELDS[:1])

    @property
    def edits_pitch_energy(self):
        return not self._is(FIELDS[1:])

    def rows(self, n):
        """float32 [n, 5]: the controls of an utterance of n phonemes."""
        out = np.empty((n, NCTL), dtype=np.float32)
        for j, name in enumerate(FIELDS):
            v = getattr(self, name)
            if isinstance(v, np.ndarray) and v.shape[0] != n:
                raise ValueError("prosody control %s: %d per-phoneme values for %d phonemes" % (name, v.shape[0], n))
            out[:, j] = v
        return out

    def __repr__(self):
        return "ProsodyControl(%s)" % ", ".join("%s=%s" % (n, getattr(self, n)) for n in FIELDS)


def per_utterance(prosody, n_utts):
    """A batch's controls: None (no control), one control for every utterance, or a list with one entry (ProsodyControl / dict / None) per
    utterance.  Returns None or a list of n_utts ProsodyControl."""
    if prosody is None:
        return None
    if isinstance(prosody, (list, tuple)):
        if len(prosody) != n_utts:
            raise ValueError("prosody: %d controls for %d utterances" % (len(prosody), n_utts))
        return [ProsodyControl.coerce(c) or ProsodyControl() for c in prosody]
    c = ProsodyControl.coerce(prosody)
    return [c] * n_utts


def check_overrides(controls, forced_dur=False, forced_f0e=False):
    """Controls edit predictions: refuse them on values the caller forced."""
    if controls is None:
        return
    if forced_dur and any(c.scales_duration for c in controls):
        raise ValueError("prosody: duration_scale != 1 with forced durations (scale the durations you pass instead)")
    if forced_f0e and any(c.edits_pitch_energy for c in controls):
        raise ValueError("prosody: a pitch / energy control with forced pitch / energy (edit the values you pass instead)")


def pack(controls, lens, t_max, out=None):
    """The [B * t_max, 5] float32 control block of the padded row layout (one row per phoneme; padding rows hold the identity)."""
    B = len(lens)
    if out is None:
        out = np.empty((B * t_max, NCTL), dtype=np.float32)
    out[:] = IDENTITY
    for b, c in enumerate(controls):
        if c is not None and b < B:
            out[b * t_max : b * t_max + int(lens[b])] = c.rows(int(lens[b]))
    return out


def duration_rule(d, duration_scale):
    """numpy restatement of the device's duration rule on predicted integer durations d: a != 1 and d >= 1 -> max(rint(fp32(d) * fp32(a)), 1)."""
    d = np.asarray(d, dtype=np.int64)
    a = np.broadcast_to(np.asarray(duration_scale, dtype=np.float32), d.shape)
    scaled = np.maximum(np.rint(d.astype(np.float32) * a), np.float32(1.0)).astype(np.int64)
    return np.where((d >= 1) & (a != np.float32(1.0)), scaled, d)


def affine_rule(v, scale, shift):
    """numpy restatement of the pitch / energy rule (float32): fmaf(v, scale, shift) where (scale, shift) != (1, 0)."""
    v = np.asarray(v, dtype=np.float32)
    s = np.broadcast_to(np.asarray(scale, dtype=np.float32), v.shape)
    b = np.broadcast_to(np.asarray(shift, dtype=np.float32), v.shape)
    fma = (v.astype(np.float64) * s.astype(np.float64) + b.astype(np.float64)).astype(np.float32)  # exact product in fp64, one rounding
    return np.where((s != 1.0) | (b != 0.0), fma, v)
