"""Text -> waveform pipeline, the part that needs no GPU: the new C entry points' argument validation through the loaded library, the numpy
statements of the PCM rule and of the capacity maps, and everything the `fcl_taco2_amd.tts` driver does before its first device call."""
import ctypes as C
import os
import wave

import numpy as np
import pytest

import fcl_taco2_amd  # noqa: F401
from fcl_taco2_amd import _lib, ops, vocoder as V
from fcl_taco2_amd import vocoder_decode as VD

NEW = ("fcl_pwg_maps_build", "fcl_pwg_gather_pad", "fcl_pwg_noise_cap", "fcl_pwg_first_conv_cap", "fcl_pwg_layer_cap_fwd", "fcl_pwg_last_cap_fwd",
       "fcl_pcm16_fwd")
A128, A16, ODD = 0x10000, 0x10010, 0x10004  # fake addresses: validation happens before any launch, nothing is dereferenced


def rc_msg(rc):
    return rc, (_lib.load().fcl_last_error() or b"").decode()


def test_new_exports_are_bound_and_the_abi_revision_is_unchanged():
    lib = _lib.load()
    assert lib.fcl_version() == 423 == _lib.ABI_VERSION
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fcl_hip.h")).read()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name) and ("int %s(" % name) in header, name
    assert (_lib.STATUS_VOCODER_CAP, _lib.STATUS_PCM_NONFINITE) == (32, 64)
    assert "FCL_STATUS_VOCODER_CAP = 32" in header and "FCL_STATUS_PCM_NONFINITE = 64" in header
    msg = ops.status_message(_lib.STATUS_VOCODER_CAP | _lib.STATUS_PCM_NONFINITE)
    assert "vocoder capacity" in msg and "non-finite" in msg and "unknown" not in msg


def maps_build(utt_frame0=A16, status=A16, batch=4, frames_cap=64, ctx=2, hop=256, seg=A16, live=A16):
    return rc_msg(_lib.load().fcl_pwg_maps_build(utt_frame0, status, batch, frames_cap, ctx, hop, A16, A16, A16, A16, A16, A16, seg, seg, live, None))


def test_maps_build_validates_its_arguments():
    assert maps_build(utt_frame0=None)[0] == -1 and maps_build(status=None)[0] == -1
    rc, msg = maps_build(live=None)
    assert rc == -1 and "null" in msg  # FCL_ERR_INVALID
    assert maps_build(batch=0)[0] == -1 and maps_build(batch=5000)[0] == -1 and maps_build(frames_cap=0)[0] == -1
    rc, msg = maps_build(hop=200)
    assert rc == -2 and "multiple of 128" in msg  # FCL_ERR_SHAPE
    rc, msg = maps_build(frames_cap=2 ** 31 // 256, hop=256)
    assert rc == -2 and "2^31" in msg
    rc, msg = maps_build(seg=ODD)
    assert rc == -3 and "aligned" in msg  # FCL_ERR_ALIGN


def layer(**kw):
    a = _lib.PwgLayer()
    a.m, a.r, a.aux, a.ksize, a.dilation, a.first_layer = 128 * 40, 64, 80, 3, 1, 1
    for n in ("seg_lo", "seg_hi", "w_conv_p", "b_conv", "w_os_p", "b_os", "skips", "kp", "pt_a", "pt_b"):
        setattr(a, n, A128)
    a.xp, a.xp_out, a.ld_pt, a.hop = A128, 2 * A128, 4, 256
    live = kw.pop("live", A16)
    for k, v in kw.items():
        setattr(a, k, v)
    return rc_msg(_lib.load().fcl_pwg_layer_cap_fwd(C.byref(a), live, None))


def test_layer_cap_fwd_validates_its_arguments():
    assert layer(live=None)[0] == -1 and layer(xp_out=None)[0] == -1 and layer(pt_a=None)[0] == -1
    rc, msg = layer(r=32)
    assert rc == -2 and "r = 64" in msg
    assert layer(ksize=5)[0] == -2 and layer(aux=128)[0] == -2 and layer(m=128 * 40 + 64)[0] == -2 and layer(xp_out=A128)[0] == -2
    rc, msg = layer(hop=192)
    assert rc == -2 and "multiple of 128" in msg
    assert layer(ld_pt=1)[0] == -2  # the frame windows do not cover the capacity
    rc, msg = layer(kp=A16)
    assert rc == -3 and "128-byte" in msg
    assert layer(xp=A16)[0] == -3
    # planes form with <= 64 auxiliary channels: no persistent kernel, hence no capacity form
    rc, msg = layer(kp=None, cp=A128, w_aux_p=A128, aux=40)
    assert rc == -2 and "persistent" in msg


def test_the_other_capacity_entries_validate_their_arguments():
    lib = _lib.load()
    assert lib.fcl_pwg_gather_pad(None, 8, A16, A16, 16, 80, A16, None) == -1
    assert lib.fcl_pwg_gather_pad(A16, 8, A16, A16, 16, 78, A16, None) == -1
    assert rc_msg(lib.fcl_pwg_gather_pad(ODD, 8, A16, A16, 16, 80, A16, None))[0] == -3
    assert lib.fcl_pwg_noise_cap(None, 16, 1, None, A16, None) == -1 and lib.fcl_pwg_noise_cap(A16, 16, 1, None, None, None) == -1
    assert lib.fcl_pwg_first_conv_cap(A16, A16, A16, A128, 128, 48, A16, None) == -1
    assert lib.fcl_pwg_first_conv_cap(A16, A16, A16, A16, 128, 64, A16, None) == -3
    assert lib.fcl_pwg_last_cap_fwd(A16, 1.0, A16, A16, A16, 0.0, A16, 128, 64, None, None) == -1
    rc, msg = rc_msg(lib.fcl_pwg_last_cap_fwd(A16, 1.0, A16, A16, A16, 0.0, A16, 128, 32, A16, None))
    assert rc == -2 and "64 skip channels" in msg
    assert lib.fcl_pwg_last_cap_fwd(ODD, 1.0, A16, A16, A16, 0.0, A16, 128, 64, A16, None) == -3
    assert lib.fcl_pcm16_fwd(None, A16, 16, None, A16, None) == -1 and lib.fcl_pcm16_fwd(A16, A16, 16, None, None, None) == -1
    rc, msg = rc_msg(lib.fcl_pcm16_fwd(ODD, A16, 16, None, A16, None))
    assert rc == -3 and "aligned" in msg
    assert lib.fcl_pcm16_fwd(A16, ODD + 2, 16, None, A16, None) == -3


# ---- the PCM rule ---------------------------------------------------------------------------------------------------------------------------
_f = np.float32
# the edge vector of the PCM rule (the GPU test of fcl_pcm16_fwd uses the same one): +-1 and their neighbours, the only float32 ties in range
# (+-0.5) and the clipped ones, values beyond +-1, +-0, denormals, near-tie values
EDGE = np.array([1.0, -1.0, np.nextafter(_f(1), _f(0)), np.nextafter(_f(1), _f(2)), np.nextafter(_f(-1), _f(0)), np.nextafter(_f(-1), _f(-2)), 0.5, -0.5, 1.5, -1.5,
                 2.5, -2.5, 2.0, -2.0, 1e30, -1e30, 0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, 0.25, 1.0 / 3.0, 32766.5 / 32767, -32767.5 / 32767],
                dtype=np.float32)


def test_pcm16_rule_writes_the_bytes_of_write_wav(tmp_path):
    """A float32 times 32767 (odd) is a tie k + 0.5 only for odd multiples of 0.5: +-0.5 (-> +-16384, the even neighbour) inside the range, +-1.5,
    +-2.5 beyond it (clipped); the rule's ties in both parities are exercised on doubles."""
    edge = EDGE
    got = V.pcm16_rule(edge)
    assert got.dtype == np.dtype("<i2")
    VD.write_wav(str(tmp_path / "e.wav"), edge, 22050)
    with wave.open(str(tmp_path / "e.wav")) as w:
        assert w.readframes(w.getnframes()) == got.tobytes()
    assert list(got[:10]) == [32767, -32767, 32767, 32767, -32767, -32767, 16384, -16384, 32767, -32768]
    assert list(got[16:22]) == [0, 0, 0, 0, 0, 0]
    ties = (np.arange(-6, 7) + 0.5) / 32767.0  # doubles: exact ties after the product for these small k
    prod = ties * 32767.0
    assert np.all(prod - np.floor(prod) == 0.5)
    assert list(V.pcm16_rule(ties)) == [-6, -4, -4, -2, -2, 0, 0, 2, 2, 4, 4, 6, 6]
    assert list(V.pcm16_rule(np.array([np.nan, np.inf, -np.inf, 0.5], dtype=np.float32))) == [0, 0, 0, 16384]


# ---- the capacity maps ----------------------------------------------------------------------------------------------------------------------
def maps_by_loop(lens, frames_cap, ctx, hop):
    """Per-utterance loop after ParallelWaveGANGenerator._maps over the slots that have frames, then the dead pseudo-utterance (index B)."""
    B = len(lens)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    live = int(offs[-1])
    pad_cap = frames_cap + 2 * ctx * (B + 1)
    pad_idx, lo, hi, keep, fu = [], [], [], [], []
    base = 0
    for u, n in enumerate(lens):
        if n == 0:
            continue
        pad_idx.append(offs[u] + np.clip(np.arange(-ctx, n + ctx), 0, n - 1))
        lo.append(np.full(n + 2 * ctx, base))
        hi.append(np.full(n + 2 * ctx, base + n + 2 * ctx))
        keep.append(np.arange(base + ctx, base + ctx + n))
        fu.append(np.full(n, u))
        base += n + 2 * ctx
    dead = frames_cap - live
    pad_idx.append(np.zeros(pad_cap - base))
    lo.append(np.full(pad_cap - base, base))
    hi.append(np.full(pad_cap - base, pad_cap))
    keep.append(np.arange(base + ctx, base + ctx + dead))
    fu.append(np.full(dead, B))
    fu = np.concatenate(fu).astype(np.int64)
    offx = np.concatenate([offs, [frames_cap]])
    cat = lambda a: np.concatenate(a).astype(np.int32)
    return dict(pad_idx=cat(pad_idx), lo=cat(lo), hi=cat(hi), keep=cat(keep), frame_utt=fu.astype(np.int32), utt_off=offx.astype(np.int32),
                seg_lo=(np.repeat(offx[fu], hop) * hop).astype(np.int32), seg_hi=(np.repeat(offx[fu + 1], hop) * hop).astype(np.int32),
                live=np.array([live, live * hop, base, sum(1 for n in lens if n)], dtype=np.int32))


def cases():
    out = [([5, 1, 3], 16), ([7, 2, 1, 9, 0, 0], 40), ([1], 1), ([0, 0, 0], 8), ([4, 4], 8), ([3, 0, 2, 0, 6], 32), ([0, 5], 5), ([64] * 8, 512)]
    rng = np.random.RandomState(0)
    for _ in range(40):
        b = int(rng.randint(1, 24))
        lens = [int(v) * int(rng.rand() < 0.8) for v in rng.randint(1, 60, size=b)]
        out.append((lens, sum(lens) + int(rng.randint(0, 3)) * int(rng.randint(0, 70)) if sum(lens) else 5))
    return out


@pytest.mark.parametrize("ctx,hop", [(2, 256), (0, 128), (3, 384)])
def test_capacity_maps_rule_equals_the_per_utterance_loop(ctx, hop):
    for lens, cap in cases():
        got = V.capacity_maps_rule(np.concatenate([[0], np.cumsum(lens)]), cap, ctx, hop)
        want = maps_by_loop(lens, cap, ctx, hop)
        assert got["ok"]
        pad_cap, m_cap = V.capacity_sizes(len(lens), cap, ctx, hop)
        for k, v in want.items():
            assert got[k].dtype == np.int32 and np.array_equal(got[k], v), (k, lens, cap)
        # every index inside its buffer, over the whole capacity
        assert got["pad_idx"].shape == (pad_cap,) and got["pad_idx"].min() >= 0 and got["pad_idx"].max() < max(cap, 1)
        assert got["pad_idx"].max() < max(sum(lens), 1)  # ... and inside the LIVE mel rows: dead rows are never a source
        assert got["lo"].min() >= 0 and got["hi"].max() <= pad_cap and np.all(got["lo"] < got["hi"])
        assert got["keep"].shape == (cap,) and got["keep"].min() >= 0 and got["keep"].max() < pad_cap and np.unique(got["keep"]).size == cap
        assert got["frame_utt"].min() >= 0 and got["frame_utt"].max() <= len(lens)
        assert got["seg_lo"].shape == (m_cap,) and got["seg_lo"].min() >= 0 and got["seg_hi"].max() <= m_cap and np.all(got["seg_lo"] < got["seg_hi"])
        assert np.all((got["lo"] <= np.arange(pad_cap)) & (np.arange(pad_cap) < got["hi"]))
        assert np.all((got["seg_lo"] <= np.arange(m_cap)) & (np.arange(m_cap) < got["seg_hi"]))


def test_capacity_maps_rule_refuses_instead_of_truncating():
    for f0, cap, status in (([0, 5, 14, 17], 16, 0), ([0, 5, 8], 16, 8), ([0, 9, 4, 12], 16, 0), ([1, 2, 3], 16, 0)):
        got = V.capacity_maps_rule(f0, cap, 2, 256, status=status)
        assert not got["ok"] and list(got["live"]) == [0, 0, 0, 0]
        assert np.all(got["frame_utt"] == len(f0) - 1) and np.all(got["seg_lo"] == 0) and np.all(got["seg_hi"] == cap * 256) and np.all(got["pad_idx"] == 0)


# ---- the driver, before its first device call -------------------------------------------------------------------------------------------------
BASE = ["--model", "m", "--model-conf", "c", "--json", "j", "--vocoder-checkpoint", "v", "--outdir", "o"]


def test_driver_arguments_and_shared_prosody_flags(capsys):
    from fcl_taco2_amd import decode as D, tts as T

    a = T.parse_args(BASE)
    assert (a.batch_size, a.nj, a.job, a.seed, a.feats_out, a.unsafe_pickle, a.max_buckets, a.vocoder_config) == (32, 1, 0, 137, None, False, 2, None)
    a = T.parse_args(BASE + ["--batch-size", "8", "--nj", "4", "--job", "3", "--feats-out", "x/feats", "--unsafe-pickle", "--duration-scale", "1.5",
                             "--pitch-shift", "0.2", "--vocoder-config", "cfg.yml", "--teacher-config", "t.json"])
    assert (a.batch_size, a.nj, a.job, a.feats_out, a.unsafe_pickle, a.vocoder_config, a.teacher_config) == (8, 4, 3, "x/feats", True, "cfg.yml", "t.json")
    ctl = D.prosody_from_args(a)
    assert ctl.duration_scale == 1.5 and ctl.pitch_shift == 0.2
    # the prosody flags are decode.py's own group, not a copy
    import argparse

    ref = argparse.ArgumentParser()
    D.add_prosody_arguments(ref)
    flags = lambda ap: sorted(o for act in ap._actions for o in act.option_strings if o not in ("-h", "--help"))
    assert set(flags(ref)) <= set(flags(T.build_parser())) and "--duration-scale" in flags(ref)
    for bad, text in ((["--job", "2", "--nj", "2"], "--job must lie in"), (["--batch-size", "0"], "--batch-size must be at least 1"),
                      (["--max-buckets", "0"], "--max-buckets"), (["--semitones", "2"], "--f0-en-stats"),
                      (["--semitones", "2", "--pitch-scale", "1.1", "--f0-en-stats", "s.npy"], "both set the pitch control")):
        with pytest.raises(SystemExit) as e:
            T.parse_args(BASE + bad)
        assert e.value.code == 2 and text in capsys.readouterr().err
    with pytest.raises(SystemExit):
        T.parse_args(BASE[2:])  # --model is required


def test_driver_batches_buckets_shards_and_caps():
    from fcl_taco2_amd import tts as T

    assert [T.bucket_of(n) for n in (1, 16, 17, 100)] == [16, 16, 32, 112]
    lengths = [5, 40, 17, 16, 3, 33, 90]
    plan = T.plan_batches(lengths, 3)
    assert plan == [(96, [6, 1, 5]), (32, [2, 3, 0]), (16, [4])]
    assert sorted(i for _, idx in plan for i in idx) == list(range(len(lengths)))
    with pytest.raises(ValueError, match="--batch-size"):
        T.plan_batches(lengths, 0)
    utts = [("u%d" % i, np.zeros(n, dtype=np.int64)) for i, n in enumerate(lengths)]
    parts = [T.shard_of(utts, 3, j) for j in range(3)]
    assert sorted(u[0] for p in parts for u in p) == sorted(u[0] for u in utts) and all(parts)
    assert max(sum(len(u[1]) for u in p) for p in parts) <= 90 + 17  # balanced by phoneme count
    assert T.vocoder_frames_cap(57600, 256) == 57600
    with pytest.raises(ValueError, match="2\\^31 samples"):
        T.vocoder_frames_cap(2 ** 23, 256)


def test_write_pcm_wav_round_trip(tmp_path):
    from fcl_taco2_amd import tts as T

    x = (np.random.RandomState(1).standard_normal(1000) * 0.3).astype(np.float32)
    T.write_pcm_wav(str(tmp_path / "a.wav"), V.pcm16_rule(x), 24000)
    VD.write_wav(str(tmp_path / "b.wav"), x, 24000)
    assert (tmp_path / "a.wav").read_bytes() == (tmp_path / "b.wav").read_bytes()


def test_capacity_synth_needs_a_device_plan():
    """No CPU fallback: the capacity entry sits on a PWGPlan, which refuses anything but a GPU device."""
    from fcl_taco2_amd import synthetic as SYN

    sd = {k: SYN.closed_form_tensor("pwg." + k, tuple(s)) for k, s in V.param_spec().items()}
    with pytest.raises(_lib.FclError):
        V.PWGPlan(sd, "cpu")
    from fcl_taco2_amd import engine

    assert issubclass(engine.SpeechRunner, engine.BatchRunner) and callable(V.CapacitySynth)


def test_layer_descriptors_are_one_chain_for_every_route():
    """vocoder.layer_chain on a stub plan of CPU tensors: the frame-rate and the upsampled-planes auxiliary operands of the one-launch block (the
    capacity form and the exact one build the same list), and the unfused operands only the exact form uses."""
    import types

    import torch

    from fcl_taco2_amd import vocoder as V

    t = lambda: torch.empty(8)
    dil = [1, 2, 4, 8]
    pl = types.SimpleNamespace(R=64, A=80, k=3, hop=256, layers=[dict(dilation=d, w_conv_p=t(), b_conv=t(), w_aux_p=t(), w_os_p=t(), b_os=t()) for d in dil])
    M, lo, hi, ld_pt = 1280, 1 << 20, 1 << 21, 3
    xp, gp, skips, kp, pt_a, pt_b, cp, x, z, o = [t() for _ in range(10)]
    p = lambda b: b.data_ptr()

    def common(layers):
        assert len(layers) == 4
        for l, (a, L) in enumerate(zip(layers, pl.layers)):
            assert (a.m, a.r, a.aux, a.ksize, a.dilation, a.first_layer) == (M, 64, 80, 3, dil[l], int(l == 0))
            assert (a.seg_lo, a.seg_hi, a.skips) == (lo, hi, p(skips))
            assert (a.w_conv_p, a.b_conv, a.w_aux_p, a.w_os_p, a.b_os) == tuple(p(L[k]) for k in ("w_conv_p", "b_conv", "w_aux_p", "w_os_p", "b_os"))

    for aux in ((kp, pt_a, pt_b, ld_pt), cp):  # the one-launch block: x lives in planes only and ping-pongs between xp and gp
        layers = V.layer_chain(pl, M, lo, hi, xp, gp, skips, aux)
        common(layers)
        for l, a in enumerate(layers):
            assert (a.xp, a.xp_out) == ((p(xp), p(gp)) if l % 2 == 0 else (p(gp), p(xp)))
            assert (a.x, a.z, a.gp, a.o) == (None, None, None, None)
            if aux is cp:
                assert (a.cp, a.kp, a.pt_a, a.pt_b, a.ld_pt, a.hop) == (p(cp), None, None, None, 0, 0)
            else:
                step = 2 * (l * 2 * 64 * ld_pt * 64)  # bytes: this block's 2R gate rows of ld_pt lines of 64 int16
                assert (a.cp, a.kp, a.pt_a, a.pt_b, a.ld_pt, a.hop) == (None, p(kp), p(pt_a) + step, p(pt_b) + step, ld_pt, 256)
    layers = V.layer_chain(pl, M, lo, hi, xp, gp, skips, cp, x, (z, o))  # three launches per block: fp32 x and its planes updated in place
    common(layers)
    for a in layers:
        assert (a.x, a.xp, a.xp_out, a.z, a.gp, a.o, a.cp, a.kp) == (p(x), p(xp), None, p(z), p(gp), p(o), p(cp), None)
