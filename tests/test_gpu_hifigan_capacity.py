"""-m gpu: the capacity form of the HiFi-GAN generator (csrc/hifigan.hip hfg_maps_kernel and the hfg_*_cap_kernel family, hifigan.CapacitySynth,
engine.SpeechRunner and the tts driver on it).  The yardstick is the exact-size path on the same packed rows, bit for bit: the cap kernels run the
exact body on the same tiles.  Every buffer a kernel writes sits between guard zones filled with a NaN bit pattern; operand rows at and beyond the
live rows hold the pattern too (whatever is read from them poisons the result) and output rows there must still hold it afterwards.  Every test
reads the library's launch record.

  1 fcl_hfg_maps_build = hifigan.capacity_maps_rule      2 each cap entry = its exact entry at m = live rows      3 CapacitySynth.run = synthesize_packed
  4 SpeechRunner on a HiFiGANGenerator      5 the tts driver with --vocoder-graph"""
import contextlib
import ctypes as C
import json
import wave

import numpy as np
import pytest
import torch

import hifigan_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAT16, PAT32 = 0x7FC1, 0x7FC12345  # a bf16 / an fp32 NaN
SLOPE = 0.1
RATE, CAP_FRAMES = 4, 96                      # 384 rows: three 128-row tiles, 3.4 unit tiles of 112 rows
LIVE_FRAMES = [0, 1, 28, 29, CAP_FRAMES]      # rows 0, 4 (less than a tile), 112 (a unit tile boundary), 116 (one frame into the second tile), all
SLOTS = 8


@pytest.fixture(scope="module")
def hfg():
    assert torch.cuda.is_available()
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib, hifigan, ops

    _lib.load()
    if not ops.planes_enabled():
        pytest.skip("FCL_PRECISION=0 / FCL_PLANES=0: the vocoder needs the pre-split operand path")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    return hifigan


def lib():
    from fcl_taco2_amd import _lib

    return _lib.load()


def chk(rc):
    from fcl_taco2_amd import _lib

    _lib.check(rc)


def stream():
    from fcl_taco2_amd import ops

    return ops._stream()


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


@contextlib.contextmanager
def launched(*names, absent=()):
    """the launches inside run the named kernels (the library's own launch record) and none of `absent`"""
    from fcl_taco2_amd import _lib

    _lib.prof_enable(True)
    try:
        yield
        torch.cuda.synchronize()
        seen = set(_lib.prof_collect())
    finally:
        _lib.prof_enable(False)
    for n in names:
        assert n in seen, (n, sorted(seen))
    for n in absent:
        assert n not in seen, (n, sorted(seen))


class Guarded(object):
    """a device buffer of n elements between two guard zones; everything starts as the NaN pattern"""

    PAD = 8192

    def __init__(self, n, dtype):
        self.n, self.dtype = int(n), dtype
        self.buf = torch.empty(self.n + 2 * self.PAD, dtype=dtype, device=DEV)
        self.wipe()
        assert self.t.data_ptr() % 128 == 0

    def wipe(self):
        self.bits().fill_(PAT16 if self.dtype == torch.int16 else PAT32)

    def bits(self):
        return self.buf if self.dtype == torch.int16 else self.buf.view(torch.int32)

    @property
    def t(self):
        return self.buf[self.PAD : self.PAD + self.n]

    def host(self):
        """the payload's bits"""
        return self.bits()[self.PAD : self.PAD + self.n].cpu().numpy().copy()

    def intact(self):
        b, p = self.bits(), PAT16 if self.dtype == torch.int16 else PAT32
        return bool((b[: self.PAD] == p).all()) and bool((b[self.PAD + self.n :] == p).all())


def lrelu32(x, slope):
    x = np.asarray(x, dtype=np.float32)
    return np.where(x >= 0, x, x * np.float32(slope)).astype(np.float32)


def taps_planes(w):
    """(Cout, Cin, k) float32 -> the planes the entry points take: tap-major [k * Cout, Cin]"""
    from fcl_taco2_amd import ops

    wd = dev(w)
    return ops.pack_planes(ops.pack_conv1d_weight(wd).reshape(w.shape[2] * w.shape[0], w.shape[1]))


def slot_lens(live):
    """`live` frames over SLOTS slots: ragged, one-frame utterances, empty slots, edges inside a tile"""
    lens, left = [], live
    for want in (1, 0, 9, 1, 17, 0, 1):
        lens.append(min(want, left))
        left -= lens[-1]
    return lens + [left]


def device_maps(lens, frames_cap, hop, status=0, starts=None):
    """fcl_hfg_maps_build into guarded buffers -> (frame_utt, utt_off, live, status word)"""
    B = len(lens) if starts is None else len(starts) - 1
    f0 = dev(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32) if starts is None else np.asarray(starts, dtype=np.int32))
    st = dev(np.array([status], dtype=np.int32))
    fu, uo, lv = Guarded(frames_cap, torch.int32), Guarded(B + 2, torch.int32), Guarded(4, torch.int32)
    with launched("hfg_maps_kernel"):
        chk(lib().fcl_hfg_maps_build(f0.data_ptr(), st.data_ptr(), B, frames_cap, hop, fu.t.data_ptr(), uo.t.data_ptr(), lv.t.data_ptr(), stream()))
    assert fu.intact() and uo.intact() and lv.intact()
    return fu, uo, lv, st


# ------------------------------------------------------------------------------------------------------------------ 1 maps kernel
def maps_cases():
    rng = np.random.RandomState(7)
    cases = [[7, 2, 1, 9, 0, 0], [0, 0, 0], [0, 5], [3], [0], [1, 0, 1]]
    for _ in range(40):
        cases.append([int(v) for v in rng.randint(0, 12, size=rng.randint(1, 9)) * (rng.rand() < 0.8)])
    return cases


@pytest.mark.parametrize("hop", [8, 256, 384])
def test_maps_kernel_equals_the_numpy_rule(hfg, hop):
    for lens in maps_cases():
        total = sum(lens)
        for frames_cap in sorted({max(total, 1), total + 5, total + 300}):  # live == capacity, a few dead frames, more than one workgroup's share
            fu, uo, lv, st = device_maps(lens, frames_cap, hop)
            want = hfg.capacity_maps_rule(np.concatenate([[0], np.cumsum(lens)]), len(lens), frames_cap, hop)
            assert np.array_equal(fu.host(), want["frame_utt"]) and np.array_equal(uo.host(), want["utt_off"]), (lens, frames_cap)
            assert np.array_equal(lv.host(), want["live"]) and int(st.item()) == 0 == want["status"]


def test_maps_kernel_refuses_instead_of_truncating(hfg):
    from fcl_taco2_amd import _lib

    B, cap = 4, 20
    for starts, status in (([0, 7, 9, 10, 21], 0), ([0, 7, 5, 10, 12], 0), ([1, 7, 9, 10, 12], 0), ([0, 7, 9, 10, 12], 4), ([0, 7, 9, 10, 21], 4)):
        fu, uo, lv, st = device_maps(None, cap, 8, status=status, starts=starts)
        want = hfg.capacity_maps_rule(starts, B, cap, 8, status=status)
        assert not want["ok"] and want["status"] == (status or _lib.STATUS_VOCODER_CAP)
        assert int(st.item()) == want["status"], (starts, status)  # the bit is set, or the incoming word is kept
        assert lv.host().tolist() == [0, 0, 0, 0] and np.array_equal(fu.host(), want["frame_utt"]) and np.array_equal(uo.host(), want["utt_off"])


# ------------------------------------------------------------------------------------------------------------------ 2 cap entries vs exact entries
class Ctx(object):
    """tables and the live record of one (live frames) case, built by the maps kernel itself"""

    def __init__(self, live):
        self.live_frames = live
        self.fu, self.uo, self.lv, _ = device_maps(slot_lens(live), CAP_FRAMES, 8)
        assert self.lv.host()[0] == live


def poisoned_rows(values, live_rows, dtype):
    """[rows, width] device tensor: `values` on the live rows, the NaN pattern at and beyond them"""
    t = dev(values).clone()
    bits = t if dtype == torch.int16 else t.view(torch.int32)
    bits[live_rows:] = PAT16 if dtype == torch.int16 else PAT32
    return t


def both_forms(outs, inouts, run_exact, run_cap, live_rows, widths, cap_names):
    """runs the exact entry at m = live rows (nothing at 0 rows: the exact entries refuse m = 0) and the cap entry on the same buffers;
    the buffers must be bit-identical, finite on the live rows, the pattern at and beyond them, guards intact"""
    def reset():
        for g in outs.values():
            g.wipe()
        for k, (g, init) in inouts.items():
            g.wipe()
            g.t.copy_(init.reshape(-1))
    reset()
    if live_rows:
        chk(run_exact())
        torch.cuda.synchronize()
    want = {k: g.host() for k, g in list(outs.items()) + [(k, v[0]) for k, v in inouts.items()]}
    reset()
    with launched(*cap_names):
        chk(run_cap())
    for k, g in list(outs.items()) + [(k, v[0]) for k, v in inouts.items()]:
        got = g.host()
        assert g.intact(), k
        assert np.array_equal(got, want[k]), (k, live_rows)
        w = widths[k]
        pat = PAT16 if g.dtype == torch.int16 else PAT32
        if k in outs:
            assert bool((got[live_rows * w :] == pat).all()), (k, "rows beyond the live rows were written")
        live = got[: live_rows * w]
        vals = live.view(np.float32) if g.dtype != torch.int16 else (live.view(np.uint16).astype(np.uint32) << 16).view(np.float32)
        assert np.isfinite(vals).all(), (k, "a dead row entered a live one")


@pytest.mark.parametrize("live", LIVE_FRAMES)
@pytest.mark.parametrize("s,cin", [(2, 64), (8, 64), (2, 512), (8, 512)])
def test_tconv_cap_equals_exact(hfg, s, cin, live):
    from fcl_taco2_amd import _lib, ops

    cx = Ctx(live)
    cout, rows_cap, rows = cin // 2, CAP_FRAMES * RATE, live * RATE
    rng = np.random.RandomState(100 + s + cin)
    x = rng.standard_normal((rows_cap, cin)).astype(np.float32)
    w = (rng.standard_normal((cin, cout, 2 * s)) / np.sqrt(cin * 2)).astype(np.float32)
    b = (0.5 * rng.standard_normal(cout)).astype(np.float32)
    xp = poisoned_rows(ops.pack_planes(dev(x)), rows, torch.int16)
    wp, bd = taps_planes(np.ascontiguousarray(np.transpose(w, (1, 0, 2)))), dev(b)
    outs = dict(y=Guarded(rows_cap * s * cout, torch.float32), yp=Guarded(rows_cap * s * (cout // 32) * 64, torch.int16))
    a = _lib.HfgTconv()
    a.cin, a.cout, a.stride, a.ksize, a.padding, a.rate_in, a.slope = cin, cout, s, 2 * s, s // 2 + s % 2, RATE, SLOPE
    a.xp, a.wp, a.bias, a.frame_utt, a.utt_off = xp.data_ptr(), wp.data_ptr(), bd.data_ptr(), cx.fu.t.data_ptr(), cx.uo.t.data_ptr()
    a.y, a.yp = outs["y"].t.data_ptr(), outs["yp"].t.data_ptr()

    def exact():
        a.m_in = rows
        return lib().fcl_hfg_tconv_fwd(C.byref(a), stream())

    def cap():
        a.m_in = rows_cap
        return lib().fcl_hfg_tconv_cap_fwd(C.byref(a), cx.lv.t.data_ptr(), stream())

    both_forms(outs, {}, exact, cap, rows, dict(y=s * cout, yp=s * (cout // 32) * 64), ["hfg_tconv_cap_kernel"])


def unit_case(c, kr, dil, live, bf16=False):
    from fcl_taco2_amd import _lib, ops

    cx = Ctx(live)
    rows_cap, rows, ld = CAP_FRAMES * RATE, live * RATE, c // 32
    rng = np.random.RandomState(200 + c + kr)
    x = rng.standard_normal((rows_cap, c)).astype(np.float32)
    w1, w2 = [(rng.standard_normal((c, c, kr)) / np.sqrt(c * kr)).astype(np.float32) for _ in range(2)]
    b1, b2 = [(0.5 * rng.standard_normal(c)).astype(np.float32) for _ in range(2)]
    cs0 = rng.standard_normal((rows_cap, c)).astype(np.float32)
    xd = poisoned_rows(x, rows, torch.float32)
    xp = poisoned_rows(ops.pack_planes(dev(lrelu32(x, SLOPE))), rows, torch.int16)
    keep = [taps_planes(w1), taps_planes(w2), dev(b1), dev(b2)]
    outs = dict(x=Guarded(rows_cap * c, torch.float32), xp=Guarded(rows_cap * ld * 64, torch.int16), csp=Guarded(rows_cap * ld * 64, torch.int16))
    if c > 128:
        outs["tp"] = Guarded(rows_cap * ld * 64, torch.int16)
    inouts = dict(cs=(Guarded(rows_cap * c, torch.float32), poisoned_rows(cs0, rows, torch.float32)))
    u = _lib.HfgUnit()
    u.c, u.ksize, u.dilation, u.rate, u.first, u.last = c, kr, dil, RATE, 0, 1
    u.slope, u.cs_scale, u.csp_slope = SLOPE, 1.0 / 3, R.OUT_SLOPE
    u.xp, u.x, u.w1p, u.w2p, u.b1, u.b2 = xp.data_ptr(), xd.data_ptr(), keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr()
    u.frame_utt, u.utt_off = cx.fu.t.data_ptr(), cx.uo.t.data_ptr()
    u.x_out, u.xp_out, u.cs, u.csp = outs["x"].t.data_ptr(), outs["xp"].t.data_ptr(), inouts["cs"][0].t.data_ptr(), outs["csp"].t.data_ptr()
    u.tp = outs["tp"].t.data_ptr() if c > 128 else None

    def exact():
        u.m = rows
        return lib().fcl_hfg_unit_fwd(C.byref(u), stream())

    def cap():
        u.m = rows_cap
        return lib().fcl_hfg_unit_cap_fwd(C.byref(u), cx.lv.t.data_ptr(), stream())

    sfx = "/bf16" if bf16 else ""
    name = ("hfg_unit_cap_kernel<%d>" % c if c <= 128 else "hfg_conv_cap_kernel") + sfx
    widths = dict(x=c, xp=ld * 64, csp=ld * 64, tp=ld * 64, cs=c)
    both_forms(outs, inouts, exact, cap, rows, widths, [name])
    return keep, xd, xp


@pytest.mark.parametrize("live", LIVE_FRAMES)
@pytest.mark.parametrize("kr,dil", [(3, 1), (11, 5)])
@pytest.mark.parametrize("c", [32, 64, 128, 256])
def test_unit_cap_equals_exact(hfg, c, kr, dil, live):
    unit_case(c, kr, dil, live)


def test_unit_cap_equals_exact_in_bf16_mode(hfg):
    from fcl_taco2_amd import ops

    with ops.gemm_mode("bf16"):
        unit_case(64, 11, 5, 29, bf16=True)
        unit_case(256, 3, 1, 29, bf16=True)


@pytest.mark.parametrize("live", LIVE_FRAMES)
def test_input_conv_cap_equals_exact(hfg, live):
    from fcl_taco2_amd import _lib, ops

    cx = Ctx(live)
    cin, cout, k, rows_cap, rows = 80, 128, 7, CAP_FRAMES * RATE, live * RATE
    rng = np.random.RandomState(300)
    x = rng.standard_normal((rows_cap, cin)).astype(np.float32)
    w, b = (rng.standard_normal((cout, cin, k)) / np.sqrt(cin * k)).astype(np.float32), (0.5 * rng.standard_normal(cout)).astype(np.float32)
    xp = poisoned_rows(ops.pack_planes(dev(x)), rows, torch.int16)
    wp, bd = taps_planes(w), dev(b)
    outs = dict(y=Guarded(rows_cap * cout, torch.float32), yp=Guarded(rows_cap * (cout // 32) * 64, torch.int16))
    a = _lib.HfgConv()
    a.cin, a.cout, a.ksize, a.dilation, a.rate, a.slope = cin, cout, k, 1, RATE, SLOPE
    a.xp, a.wp, a.bias, a.frame_utt, a.utt_off = xp.data_ptr(), wp.data_ptr(), bd.data_ptr(), cx.fu.t.data_ptr(), cx.uo.t.data_ptr()
    a.y, a.yp = outs["y"].t.data_ptr(), outs["yp"].t.data_ptr()

    def exact():
        a.m = rows
        return lib().fcl_hfg_conv_fwd(C.byref(a), stream())

    def cap():
        a.m = rows_cap
        return lib().fcl_hfg_conv_cap_fwd(C.byref(a), cx.lv.t.data_ptr(), stream())

    both_forms(outs, {}, exact, cap, rows, dict(y=cout, yp=(cout // 32) * 64), ["hfg_conv_cap_kernel"])


@pytest.mark.parametrize("live", LIVE_FRAMES)
def test_output_conv_cap_equals_exact(hfg, live):
    from fcl_taco2_amd import ops

    cx = Ctx(live)
    c, k, rows_cap, rows = 32, 7, CAP_FRAMES * RATE, live * RATE
    rng = np.random.RandomState(400)
    a32 = lrelu32(rng.standard_normal((rows_cap, c)).astype(np.float32), R.OUT_SLOPE)
    w, b = (rng.standard_normal((1, c, k)) / np.sqrt(c * k)).astype(np.float32), (0.5 * rng.standard_normal(1)).astype(np.float32)
    ap = poisoned_rows(ops.pack_planes(dev(a32)), rows, torch.int16)
    wd, bd = ops.pack_conv1d_weight(dev(w)), dev(b)
    outs = dict(wav=Guarded(rows_cap, torch.float32))
    args = lambda m: (ap.data_ptr(), wd.data_ptr(), bd.data_ptr(), cx.fu.t.data_ptr(), cx.uo.t.data_ptr(), RATE, outs["wav"].t.data_ptr(), m, c, 1, k)
    both_forms(outs, {}, lambda: lib().fcl_hfg_out_fwd(*(args(rows) + (stream(),))),
               lambda: lib().fcl_hfg_out_cap_fwd(*(args(rows_cap) + (cx.lv.t.data_ptr(), stream()))), rows, dict(wav=1), ["hfg_out_cap_kernel"])


# ------------------------------------------------------------------------------------------------------------------ 3 CapacitySynth
def make_generator(hfg, key, **over):
    cfg = dict(dict(v1=R.V1, small=R.SMALL)[key], **over)
    sd, mels = R.generator_inputs(R.SEEDS[key], R.GENERATOR_LENS, cfg)
    return cfg, mels, hfg.HiFiGANGenerator(hfg.HiFiGANPlan(sd, DEV, R.plan_cfg(cfg)))


def run_capacity(hfg, gen, synth, slot_mels, status=0):
    """one run of `synth` on the slots' mels (None = an empty slot) against synthesize_packed on the same packed rows"""
    from fcl_taco2_amd import vocoder

    hop, F = gen.plan.hop, synth.frames_cap
    lens = [0 if m is None else m.shape[0] for m in slot_mels]
    live = sum(lens)
    rows = np.full((F, gen.plan.A), np.nan, dtype=np.float32)  # NaN in the dead mel rows
    rows[:live] = np.concatenate([m for m in slot_mels if m is not None])
    mel = dev(rows)
    f0 = dev(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32))
    st = dev(np.array([status], dtype=np.int32))
    synth.wav.view(torch.int32).fill_(PAT32)
    synth.pcm.fill_(PAT16)
    names = ["hfg_maps_kernel", "hfg_conv_cap_kernel", "hfg_tconv_cap_kernel", "hfg_out_cap_kernel", "pwg_pcm16_kernel", "hfg_unit_cap_kernel<32>",
             "hfg_unit_cap_kernel<64>"]
    mem = torch.cuda.memory_allocated()
    with launched(*names, absent=["hfg_unit_kernel<32>", "hfg_unit_kernel<64>", "hfg_tconv_kernel", "hfg_out_kernel"]):
        synth.run(mel, f0, st, seed_dev=None)
    assert torch.cuda.memory_allocated() == mem  # run allocates nothing
    want_maps = hfg.capacity_maps_rule(f0.cpu().numpy(), len(lens), F, hop)
    assert np.array_equal(synth.live.cpu().numpy(), want_maps["live"]) and int(st.item()) == 0
    _, flat = gen.synthesize_packed(mel[:live].clone(), [n for n in lens if n], return_flat=True)
    n = live * hop
    wav = synth.wav.cpu().numpy()
    assert np.array_equal(wav[:n], flat.cpu().numpy()) and np.abs(wav[:n]).max() > 0
    assert bool((synth.wav.view(torch.int32)[n:] == PAT32).all()) and bool((synth.pcm[n:] == PAT16).all())
    assert np.array_equal(synth.pcm[:n].cpu().numpy(), vocoder.pcm16_rule(flat.cpu().numpy()))


@pytest.mark.parametrize("extra", [0, 5])
@pytest.mark.parametrize("key", ["small", "v1"])
def test_capacity_synth_equals_synthesize_packed(hfg, key, extra):
    cfg, mels, gen = make_generator(hfg, key)
    slots = mels[:3] + [None, None] + mels[3:]  # 8 slots, two empty ones in the middle
    F = sum(R.GENERATOR_LENS) + extra
    synth = gen.capacity_synth(len(slots), F)
    assert isinstance(synth, hfg.CapacitySynth) and synth.M == F * gen.plan.hop and synth.pcm.shape[0] == synth.M == synth.wav.shape[0]
    want = hfg.capacity_nbytes(R.plan_cfg(cfg), len(slots), F)
    print("%s frames_cap %d: nbytes %d, capacity_nbytes %d" % (key, F, synth.nbytes, want))
    assert want <= synth.nbytes <= want + 512 * 16  # allocator rounding: 512 B per tensor, at most 16 tensors
    run_capacity(hfg, gen, synth, slots)
    run_capacity(hfg, gen, synth, [mels[1], None, mels[2], mels[4], None, None, mels[5], None])  # the same instance, a shorter batch
    run_capacity(hfg, gen, synth, slots)


def test_capacity_synth_refuses_two_output_channels(hfg):
    from fcl_taco2_amd import _lib

    _, _, gen = make_generator(hfg, "small", out_channels=2)
    with pytest.raises(_lib.FclError, match="out_channels = 2"):
        gen.capacity_synth(4, 16)


# ------------------------------------------------------------------------------------------------------------------ 4 SpeechRunner
def test_speech_runner_with_a_hifigan_generator(hfg):
    """capture, then replays with different batches: the runner's own mel and frames() through synthesize_packed and pcm16_rule give waveforms() bit
    for bit.  A replay enqueues through the graph, so the library's launch record (host side) must hold no exact unit kernel then; that the
    captured chain is the cap kernels' is read from an eager run of the same synth."""
    from fcl_taco2_amd import _lib, engine, hparams as HP, ops, synthetic as SYN, vocoder
    from fcl_taco2_amd.plan import SynthesisPlan

    _, _, gen = make_generator(hfg, "small")
    hp = HP.student_hparams(dropout_rate=0.0)
    plan = SynthesisPlan(SYN.positive_duration_head(SYN.closed_form_state_dict(HP.param_spec(hp))), hp, DEV)
    B, T_cap = 6, 32
    xs, _ = SYN.batch_c2(hp.idim, batch=B, t_lo=10, t_hi=T_cap, seed=9)
    xs2, _ = SYN.batch_c2(hp.idim, batch=4, t_lo=5, t_hi=24, seed=21)
    maps = []
    for b_ in (xs, xs2):
        _, _, inter = engine.run(plan, engine.prepare(plan, b_), ops.DROP_NONE, return_intermediates=True)
        maps.append(inter["maps"])
    caps = engine.Caps.for_batches(maps, slack_steps=2)
    r = engine.SpeechRunner(plan, gen, B, T_cap, caps, seed=5)
    assert isinstance(r.synth, hfg.CapacitySynth) and r.synth.frames_cap == caps.frames and r.hop == 8
    graph = r.graph
    exact_units = ["hfg_unit_kernel<32>", "hfg_unit_kernel<64>", "hfg_tconv_kernel", "hfg_out_kernel"]
    totals = []
    for batch in (xs, xs2, xs):
        r.load(batch)
        with launched(absent=exact_units):
            r.replay()
            pcm = r.waveforms()
        frames = r.frames()
        total = sum(frames)
        totals.append(total)
        assert r.graph is graph and len(pcm) == len(batch) and min(frames) >= 1
        want = gen.synthesize_packed(r.mel[:total].clone(), frames)
        for p, w in zip(pcm, want):
            assert p.dtype == np.int16 and np.array_equal(p, vocoder.pcm16_rule(w.cpu().numpy())) and np.abs(p).max() > 0
    assert totals[0] == totals[2] != totals[1]
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    with launched("hfg_maps_kernel", "hfg_conv_cap_kernel", "hfg_tconv_cap_kernel", "hfg_unit_cap_kernel<32>", "hfg_unit_cap_kernel<64>", "hfg_out_cap_kernel",
                  absent=exact_units):
        r.synth.run(r.mel, r._frames.utt_frame0, st)
    # the vocoder's own capacity: exceeded while the synthesis capacities hold -> reported, nothing truncated
    small = engine.SpeechRunner(plan, gen, B, T_cap, caps, voc_frames_cap=totals[0] - 1, seed=5)
    small.load(xs)
    small.replay()
    with pytest.raises(_lib.FclError, match="vocoder capacity"):
        small.waveforms()
    small.load(xs2)  # a batch that fits runs through the same graph afterwards
    small.replay()
    assert sum(p.shape[0] for p in small.waveforms()) == 8 * totals[1]


# ------------------------------------------------------------------------------------------------------------------ 5 driver
HFG_YML = """sampling_rate: 24000
generator_type: HiFiGANGenerator
generator_params:
  channels: 128
  upsample_scales: [4, 2]
  upsample_kernel_sizes: [8, 4]
  nonlinear_activation_params: {negative_slope: 0.1}
"""


def _read_wav(path):
    with wave.open(str(path)) as f:
        return (f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()), np.frombuffer(f.readframes(f.getnframes()), dtype="<i2")


def test_tts_driver_vocoder_graph_flag(hfg, tmp_path):
    """the setup of test_gpu_hifigan.py's driver test: with --vocoder-graph later batches run in the captured graph, without it every batch is eager"""
    from fcl_taco2_amd import hparams as HP, synthetic as SYN, tts as TTS, vocoder, vocoder_decode as V
    from fcl_taco2_amd.kaldi_io import read_scp

    sd = R.random_state_dict(np.random.RandomState(R.SEEDS["drivers"]), R.SMALL)
    stored = R.with_weight_norm(sd, np.random.RandomState(R.SEEDS["drivers"] + 1))
    torch.save({"model": {"generator": {k: torch.from_numpy(v) for k, v in stored.items()}}}, tmp_path / "hifigan.pkl")
    (tmp_path / "config.yml").write_text(HFG_YML)
    hp = HP.student_hparams(dropout_rate=0.0)
    msd = {k: torch.from_numpy(np.asarray(v)) for k, v in SYN.closed_form_state_dict(HP.param_spec(hp, HP.teacher_hparams(), True)).items()}
    msd["duration_predictor.linear.weight"] = torch.zeros_like(msd["duration_predictor.linear.weight"])
    msd["duration_predictor.linear.bias"] = torch.full((1,), float(np.log(4.0)))  # every phoneme predicts 3 frames
    torch.save({"model": msd, "optimizer": {}}, tmp_path / "snapshot.ep.1")
    args = dict(model_module="nets.knowledge_distillation.e2e_tts_tacotron2_sa_kd_student:Tacotron2_sa", embed_dim=256, eunits=256,
                econv_chans=256, dunits=256, postnet_chans=128, use_residual=False, use_masking=True, dropout_rate=0.0, share_proj=True)
    (tmp_path / "model.json").write_text(json.dumps([80, 80, args]))
    (tmp_path / "teacher.json").write_text(json.dumps([80, 80, dict(use_residual=False)]))
    rng = np.random.RandomState(3)
    utts = {"u%02d" % i: {"output": [{"tokenid": " ".join(map(str, rng.randint(1, 80, size=rng.randint(5, 40))))}]} for i in range(7)}
    (tmp_path / "data.json").write_text(json.dumps({"utts": utts}))
    lens = {k: len(v["output"][0]["tokenid"].split()) for k, v in utts.items()}
    base = ["--model", str(tmp_path / "snapshot.ep.1"), "--model-conf", str(tmp_path / "model.json"), "--teacher-config", str(tmp_path / "teacher.json"),
            "--json", str(tmp_path / "data.json"), "--vocoder-checkpoint", str(tmp_path / "hifigan.pkl"), "--batch-size", "3", "--verbose", "0", "--seed", "11"]
    res = TTS.main(base + ["--outdir", str(tmp_path / "wav"), "--feats-out", str(tmp_path / "feats"), "--vocoder-graph"])
    assert res["graph_batches"] >= 1 and res["graph_batches"] + res["eager_batches"] + res["redone_batches"] == 3 == len(res["batches"])
    assert res["samples"] == 8 * 3 * sum(lens.values())
    mels = read_scp(str(tmp_path / "feats.scp"))
    gen, _ = V.build_generator(str(tmp_path / "hifigan.pkl"), DEV)
    for route, ids, _seed in res["batches"]:
        rows = torch.from_numpy(np.concatenate([mels[k] for k in ids])).to(DEV)
        want = gen.synthesize_packed(rows, [mels[k].shape[0] for k in ids])
        for k, w in zip(ids, want):
            hdr, pcm = _read_wav(tmp_path / "wav" / (k + "_gen.wav"))
            assert hdr == (1, 2, 24000, 8 * 3 * lens[k]) and np.array_equal(pcm, vocoder.pcm16_rule(w.cpu().numpy())), (route, k)
    assert any(route == "graph" for route, _, _ in res["batches"])
    with launched("hfg_unit_kernel<32>", "hfg_unit_kernel<64>", "hfg_tconv_kernel", "hfg_out_kernel", absent=["hfg_maps_kernel", "hfg_unit_cap_kernel<32>"]):
        res2 = TTS.main(base + ["--outdir", str(tmp_path / "wav2")])
    assert res2["eager_batches"] == 3 and res2["graph_batches"] == 0 and res2["redone_batches"] == 0
