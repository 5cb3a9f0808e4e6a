"""CPU-only checks of prosody control: ProsodyControl validation and unit conversion, the duration rule, the decode flags, and the argument
validation of the two ctl entries of the C ABI (which returns before any HIP call)."""
import argparse
import json
import math

import numpy as np
import pytest

import fcl_taco2_amd  # noqa: F401
from fcl_taco2_amd import prosody as P


def test_validation():
    for bad in (0.0, -1.0, 8.0001, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            P.ProsodyControl(duration_scale=bad)
    with pytest.raises(ValueError):
        P.ProsodyControl(duration_scale=np.array([1.0, 0.0, 2.0]))
    for f in ("pitch_scale", "pitch_shift", "energy_scale", "energy_shift"):
        with pytest.raises(ValueError):
            P.ProsodyControl(**{f: float("nan")})
        with pytest.raises(ValueError):
            P.ProsodyControl(**{f: np.array([0.0, float("inf")])})
    with pytest.raises(ValueError):
        P.ProsodyControl(pitch_shift=np.zeros((2, 2)))
    with pytest.raises(ValueError):
        P.ProsodyControl.coerce({"speed": 2.0})
    assert P.ProsodyControl(duration_scale=8.0).scales_duration
    assert P.ProsodyControl().is_identity and not P.ProsodyControl(energy_shift=0.5).is_identity
    with pytest.raises(ValueError):  # per-phoneme arrays must cover the utterance
        P.ProsodyControl(pitch_shift=np.zeros(3)).rows(4)


def test_overrides_are_refused():
    with pytest.raises(ValueError):
        P.check_overrides([P.ProsodyControl(duration_scale=2.0)], forced_dur=True)
    with pytest.raises(ValueError):
        P.check_overrides([P.ProsodyControl(pitch_shift=0.1)], forced_f0e=True)
    with pytest.raises(ValueError):
        P.check_overrides([P.ProsodyControl(energy_scale=1.5)], forced_f0e=True)
    P.check_overrides([P.ProsodyControl(pitch_shift=0.1)], forced_dur=True)  # controls on what is still predicted are fine
    P.check_overrides([P.ProsodyControl(duration_scale=0.5)], forced_f0e=True)


def test_from_units():
    stats = np.array([5.1, 0.27, 0.8, 1.9])
    c = P.ProsodyControl.from_units(stats=stats, semitones=2.0, pitch_range=1.3, energy_gain=1.5, duration_scale=0.9)
    assert c.pitch_shift == pytest.approx(2.0 * math.log(2.0) / (12.0 * 0.27), rel=1e-12)
    assert c.pitch_scale == 1.3 and c.energy_scale == 1.5 and c.duration_scale == 0.9
    assert c.energy_shift == pytest.approx(0.5 * 0.8 / 1.9, rel=1e-12)
    assert P.ProsodyControl.from_units(pitch_range=0.5).pitch_scale == 0.5  # a range factor needs no statistics
    with pytest.raises(ValueError):
        P.ProsodyControl.from_units(semitones=1.0)
    with pytest.raises(ValueError):
        P.ProsodyControl.from_units(energy_gain=2.0)
    with pytest.raises(ValueError):
        P.ProsodyControl.from_units(stats=[1.0, 0.0, 1.0, 1.0], semitones=1.0)


def test_duration_rule_table():
    rows = [  # (d, alpha, expected)
        (3, 0.5, 2), (5, 0.5, 2), (1, 0.1, 1), (3, 1.5, 4),  # the worked examples (1.5 and 2.5 round half to even)
        (7, 0.5, 4), (9, 0.5, 4), (2, 0.25, 1), (4, 0.375, 2),  # more ties
        (0, 0.5, 0), (0, 3.0, 0),  # a predicted 0 stays 0
        (1, 0.01, 1), (1, 0.4, 1), (1, 8.0, 8),  # never 0 from scaling
        (6, 1.0, 6), (0, 1.0, 0), (13, 2.0, 26),
    ]
    d = np.array([r[0] for r in rows])
    a = np.array([r[1] for r in rows], dtype=np.float32)
    assert P.duration_rule(d, a).tolist() == [r[2] for r in rows]
    assert P.duration_rule(np.array([3, 3]), 0.1).tolist() == [1, 1]
    assert P.duration_rule(np.array([3]), 2.0).dtype == np.int64


def test_pack_layout():
    cs = [P.ProsodyControl(duration_scale=2.0), None, P.ProsodyControl(pitch_shift=np.array([0.1, 0.2, 0.3]))]
    blk = P.pack(cs, [2, 1, 3], 4)
    assert blk.shape == (12, 5) and blk.dtype == np.float32
    assert np.array_equal(blk[0], [2, 1, 0, 1, 0]) and np.array_equal(blk[1], [2, 1, 0, 1, 0])
    assert np.array_equal(blk[2:8], np.tile(P.IDENTITY, (6, 1)))  # padding rows and the uncontrolled utterance: identity
    assert np.allclose(blk[8:11, 2], [0.1, 0.2, 0.3]) and np.array_equal(blk[11], P.IDENTITY)
    assert P.per_utterance(None, 3) is None
    assert len(P.per_utterance({"duration_scale": 2.0}, 3)) == 3
    with pytest.raises(ValueError):
        P.per_utterance([None], 2)


def _parse(argv):
    from fcl_taco2_amd import decode as D

    ap = argparse.ArgumentParser()
    D.add_prosody_arguments(ap)
    return D, ap.parse_args(argv)


def test_decode_flags(tmp_path):
    D, a = _parse([])
    assert D.prosody_from_args(a) is None
    D, a = _parse(["--duration-scale", "2", "--pitch-shift", "0.25"])
    c = D.prosody_from_args(a)
    assert c.duration_scale == 2.0 and c.pitch_shift == 0.25 and c.energy_scale == 1.0
    D, a = _parse(["--semitones", "2"])
    with pytest.raises(ValueError, match="f0-en-stats"):
        D.prosody_from_args(a)
    D, a = _parse(["--energy-gain", "2"])
    with pytest.raises(ValueError, match="f0-en-stats"):
        D.prosody_from_args(a)
    stats = tmp_path / "f0_en_stats.npy"
    np.save(stats, np.array([5.0, 0.25, 1.0, 2.0]))
    D, a = _parse(["--semitones", "2", "--energy-gain", "1.5", "--f0-en-stats", str(stats)])
    c = D.prosody_from_args(a)
    assert c.pitch_shift == pytest.approx(2 * math.log(2) / (12 * 0.25)) and c.energy_shift == pytest.approx(0.5 * 1.0 / 2.0)
    D, a = _parse(["--semitones", "2", "--pitch-shift", "0.1", "--f0-en-stats", str(stats)])
    with pytest.raises(ValueError):
        D.prosody_from_args(a)
    D, a = _parse(["--duration-scale", "9"])
    with pytest.raises(ValueError):
        D.prosody_from_args(a)
    pj = tmp_path / "prosody.json"
    pj.write_text(json.dumps({"u1": {"duration_scale": 0.5}, "u2": {"pitch_shift": 1.0}}))
    D, a = _parse(["--duration-scale", "2", "--prosody-json", str(pj)])
    m = D.prosody_from_args(a, ["u1", "u2", "u3"])
    assert m["u1"].duration_scale == 0.5 and m["u2"].duration_scale == 2.0 and m["u2"].pitch_shift == 1.0 and m["u3"].duration_scale == 2.0
    pj.write_text(json.dumps({"u1": {"tempo": 0.5}}))
    D, a = _parse(["--prosody-json", str(pj)])
    with pytest.raises(ValueError):
        D.prosody_from_args(a)


def test_decode_main_rejects_semitones_without_stats(tmp_path):
    from fcl_taco2_amd import decode as D

    with pytest.raises(SystemExit):  # argparse error before any model is loaded
        D.main(["--model", str(tmp_path / "m"), "--model-conf", str(tmp_path / "c"), "--json", str(tmp_path / "j"), "--out", str(tmp_path / "o"),
                "--semitones", "2"])


def test_plugin_args_namespace():
    from fcl_taco2_amd.nets.base import prosody_from_args

    assert prosody_from_args(None) is None
    assert prosody_from_args(argparse.Namespace(threshold=0.5)) is None  # the reference's own args: no control
    assert prosody_from_args(argparse.Namespace(duration_scale=1.0)) is None
    c = prosody_from_args(argparse.Namespace(duration_scale=2.0, pitch_shift=0.5))
    assert c.duration_scale == 2.0 and c.pitch_shift == 0.5 and c.energy_scale == 1.0


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from fcl_taco2_amd import _lib

    return _lib.load()


def test_cabi_ctl_argument_validation(lib):
    import ctypes as C

    from fcl_taco2_amd import _lib

    assert _lib.ABI_VERSION == 423 and lib.fcl_version() == 423
    x, o, ctl = C.c_void_p(64), C.c_void_p(128), C.c_void_p(256)  # never dereferenced: every call below fails validation first
    rc = lib.fcl_duration_round_ctl_fwd(None, o, 4, 0, 1.0, None, None, 0, 1, None)
    assert rc == -1 and b"null" in lib.fcl_last_error()
    assert lib.fcl_duration_round_ctl_fwd(x, None, 4, 0, 1.0, None, None, 0, 1, None) == -1
    assert lib.fcl_duration_round_ctl_fwd(x, o, -1, 0, 1.0, None, None, 0, 1, None) == -1
    assert lib.fcl_duration_round_ctl_fwd(x, o, 4, 0, 1.0, None, ctl, 4, 1, None) == -1 and b"ctl_ld" in lib.fcl_last_error()
    assert lib.fcl_duration_round_ctl_fwd(x, o, 4, 0, 1.0, None, ctl, 5, 0, None) == -1 and b"ctl_row_div" in lib.fcl_last_error()
    assert lib.fcl_duration_round_ctl_fwd(x, o, 0, 0, 1.0, None, ctl, 5, 1, None) == 0  # n = 0: nothing to launch

    w = C.c_void_p(512)
    full = lambda **kw: [kw.get(k, d) for k, d in (("hs", w), ("p", x), ("e", x), ("wp", w), ("bp", w), ("we", w), ("be", w), ("lo", w), ("hi", w),
                                                     ("ctl", ctl), ("ld", 5), ("div", 1), ("out", o), ("pe", None), ("ee", None), ("po", None),
                                                     ("eo", None), ("m", 4), ("c", 8), ("k", 3))] + [None]
    f = lib.fcl_variance_embed_add_ctl_fwd
    assert f(*full(p=None)) == -1 and b"null" in lib.fcl_last_error()
    assert f(*full(e=None)) == -1
    assert f(*full(ld=4)) == -1 and b"ctl_ld" in lib.fcl_last_error()
    assert f(*full(div=0)) == -1
    assert f(*full(out=None)) == -1 and b"no output" in lib.fcl_last_error()
    assert f(*full(wp=None)) == -1
    assert f(*full(lo=None)) == -1
    assert f(*full(k=2)) == -1
    assert f(*full(hs=None)) == -1 and b"hs" in lib.fcl_last_error()
    assert f(*full(out=None, po=x)) == -1 and b"alias" in lib.fcl_last_error()
    assert f(*full(m=0)) == 0  # m = 0: nothing to launch
    assert f(*full(m=0, out=None, po=o, wp=None, lo=None, hs=None)) == 0  # scalars-only form: no weights or segments needed
