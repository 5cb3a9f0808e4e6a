"""No GPU: the capacity form of the HiFi-GAN generator up to the device -- the five exports and their argument validation (fake addresses: every
refusal returns before any HIP call), the numpy rule of the maps kernel against a plain per-utterance loop, the byte count of the shared stage
buffers, and the driver's flag.  tests/test_gpu_hifigan_capacity.py runs the kernels."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import hifigan_ref as R
from conftest import ROOT

NEW = ["fcl_hfg_maps_build", "fcl_hfg_conv_cap_fwd", "fcl_hfg_tconv_cap_fwd", "fcl_hfg_unit_cap_fwd", "fcl_hfg_out_cap_fwd"]
P = 1 << 20  # a fake, 128-byte aligned address: validation never dereferences
INVALID, SHAPE, ALIGN, WORKSPACE = -1, -2, -3, -5


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from fcl_taco2_amd import _lib

    return _lib.load()


def L():
    from fcl_taco2_amd import _lib

    return _lib


def fill(a, names):
    for n in names:
        setattr(a, n, P)
    return a


def conv_args():
    a = fill(L().HfgConv(), ("xp", "wp", "bias", "frame_utt", "utt_off", "y"))
    a.m, a.cin, a.cout, a.ksize, a.dilation, a.rate = 4, 64, 32, 3, 1, 1
    return a


def tconv_args():
    t = fill(L().HfgTconv(), ("xp", "wp", "bias", "frame_utt", "utt_off", "y"))
    t.m_in, t.cin, t.cout, t.stride, t.ksize, t.padding, t.rate_in = 4, 64, 32, 2, 4, 1, 1
    return t


def unit_args():
    u = fill(L().HfgUnit(), ("xp", "x", "w1p", "b1", "w2p", "b2", "frame_utt", "utt_off", "x_out"))
    u.m, u.c, u.ksize, u.dilation, u.rate = 4, 64, 3, 1, 1
    u.xp_out = 2 * P
    return u


def test_exports_header_and_version(lib):
    _lib = L()
    header = open(os.path.join(ROOT, "include", "fcl_hip.h")).read()
    for n in NEW:
        assert n in _lib.SIGNATURES and getattr(lib, n) is not None
        assert re.search(r"^int %s\(" % n, header, flags=re.M), n
    assert lib.fcl_version() == 423 == _lib.ABI_VERSION and "#define FCL_ABI_VERSION 423" in header


def test_maps_build_validation(lib):
    err = lib.fcl_last_error
    ok = [P, P, 4, 100, 8, P, P, P, None]
    for i in (0, 1, 5, 6, 7):  # null utt_frame0 / status / frame_utt / utt_off / live
        bad = list(ok)
        bad[i] = None
        assert lib.fcl_hfg_maps_build(*bad) == INVALID and b"null" in err(), i
    for batch in (0, 1025):
        assert lib.fcl_hfg_maps_build(P, P, batch, 100, 8, P, P, P, None) == INVALID and b"batch" in err()
    assert lib.fcl_hfg_maps_build(P, P, 4, 0, 8, P, P, P, None) == INVALID
    assert lib.fcl_hfg_maps_build(P, P, 4, 2 ** 31 // 256, 256, P, P, P, None) == SHAPE and b"2^31" in err()


def test_conv_cap_validation(lib):
    err, f = lib.fcl_last_error, lib.fcl_hfg_conv_cap_fwd
    assert f(C.byref(conv_args()), None, None) == INVALID and b"hfg_conv_cap_fwd: null" in err()
    assert f(None, P, None) == INVALID
    a = conv_args()
    a.frame_utt = None
    assert f(C.byref(a), P, None) == INVALID and b"null" in err()
    a = conv_args()
    a.cout = 48
    assert f(C.byref(a), P, None) == SHAPE and b"multiple of 32" in err()
    a = conv_args()
    a.ksize = 4
    assert f(C.byref(a), P, None) == SHAPE and b"kernel size" in err()
    a = conv_args()
    a.ksize = 13
    assert f(C.byref(a), P, None) == SHAPE
    a = conv_args()
    a.xp = P + 64
    assert f(C.byref(a), P, None) == ALIGN and b"128-byte" in err()
    a = conv_args()
    a.y = P + 4
    assert f(C.byref(a), P, None) == ALIGN


def test_tconv_cap_validation(lib):
    err, f = lib.fcl_last_error, lib.fcl_hfg_tconv_cap_fwd
    assert f(C.byref(tconv_args()), None, None) == INVALID and b"hfg_tconv_cap_fwd: null" in err()
    t = tconv_args()
    t.utt_off = None
    assert f(C.byref(t), P, None) == INVALID
    t = tconv_args()
    t.ksize = 3
    assert f(C.byref(t), P, None) == SHAPE and b"multiple of the stride" in err()
    t = tconv_args()
    t.ksize, t.padding = 8, 1
    assert f(C.byref(t), P, None) == SHAPE and b"padding" in err()
    t = tconv_args()
    t.cin = 48
    assert f(C.byref(t), P, None) == SHAPE and b"multiples of 32" in err()
    t = tconv_args()
    t.wp = P + 16
    assert f(C.byref(t), P, None) == ALIGN and b"128-byte" in err()


def test_unit_cap_validation(lib):
    err, f = lib.fcl_last_error, lib.fcl_hfg_unit_cap_fwd
    assert f(C.byref(unit_args()), None, None) == INVALID and b"hfg_unit_cap_fwd: null" in err()
    u = unit_args()
    u.frame_utt = None
    assert f(C.byref(u), P, None) == INVALID
    u = unit_args()
    u.c = 48
    assert f(C.byref(u), P, None) == SHAPE and b"multiple of 32" in err()
    u = unit_args()
    u.ksize = 9
    assert f(C.byref(u), P, None) == SHAPE and b"kernel size" in err()
    u = unit_args()
    u.dilation = 6
    assert f(C.byref(u), P, None) == SHAPE
    u = unit_args()
    u.c = 256  # one launch per convolution: needs the workspace
    assert f(C.byref(u), P, None) == WORKSPACE and b"workspace tp" in err()
    u = unit_args()
    u.xp_out = u.xp
    assert f(C.byref(u), P, None) == INVALID and b"xp_out must not be xp" in err()
    u = unit_args()
    u.last = 1  # the last unit of a block without the stage sum
    assert f(C.byref(u), P, None) == INVALID and b"stage sum" in err()
    u = unit_args()
    u.x = P + 8
    assert f(C.byref(u), P, None) == ALIGN and b"16-byte" in err()
    u = unit_args()
    u.w1p = P + 32
    assert f(C.byref(u), P, None) == ALIGN


def test_out_cap_validation(lib):
    err, f = lib.fcl_last_error, lib.fcl_hfg_out_cap_fwd
    assert f(P, P, P, P, P, 1, P, 4, 32, 1, 7, None, None) == INVALID and b"hfg_out_cap_fwd: null" in err()
    assert f(P, P, P, None, P, 1, P, 4, 32, 1, 7, P, None) == INVALID
    assert f(P, P, P, P, P, 1, P, 4, 48, 1, 7, P, None) == SHAPE and b"multiple of 32" in err()
    assert f(P, P, P, P, P, 1, P, 4, 32, 5, 7, P, None) == SHAPE
    assert f(P, P, P, P, P, 1, P, 4, 32, 1, 6, P, None) == SHAPE
    assert f(P + 64, P, P, P, P, 1, P, 4, 32, 1, 7, P, None) == ALIGN and b"128-byte" in err()


def test_exact_fp32_mode_refuses_every_cap_entry():
    """FCL_PRECISION=0 / FCL_PLANES=0 is read once per process: a child process"""
    code = """
import sys
sys.path.insert(0, %r)
import ctypes as C
import fcl_taco2_amd
from fcl_taco2_amd import _lib
lib = _lib.load()
P = 1 << 20
def fill(a, names):
    for n in names:
        setattr(a, n, P)
    return a
t = fill(_lib.HfgTconv(), ("xp", "wp", "bias", "frame_utt", "utt_off", "y"))
t.m_in, t.cin, t.cout, t.stride, t.ksize, t.padding, t.rate_in = 4, 64, 32, 2, 4, 1, 1
u = fill(_lib.HfgUnit(), ("xp", "x", "w1p", "b1", "w2p", "b2", "frame_utt", "utt_off", "x_out"))
u.m, u.c, u.ksize, u.dilation, u.rate = 4, 64, 3, 1, 1
c = fill(_lib.HfgConv(), ("xp", "wp", "bias", "frame_utt", "utt_off", "y"))
c.m, c.cin, c.cout, c.ksize, c.dilation, c.rate = 4, 64, 32, 3, 1, 1
for rc in (lib.fcl_hfg_conv_cap_fwd(C.byref(c), P, None), lib.fcl_hfg_tconv_cap_fwd(C.byref(t), P, None), lib.fcl_hfg_unit_cap_fwd(C.byref(u), P, None),
           lib.fcl_hfg_out_cap_fwd(P, P, P, P, P, 1, P, 4, 32, 1, 7, P, None)):
    assert rc == -1 and b"FCL_PRECISION=0" in lib.fcl_last_error(), (rc, lib.fcl_last_error())
print("REFUSED")
""" % ROOT
    for var in ("FCL_PRECISION", "FCL_PLANES"):
        env = dict(os.environ, **{var: "0"})
        p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and "REFUSED" in p.stdout, (var, p.stdout[-2000:], p.stderr[-2000:])


# ---------------------------------------------------------------------------------------------------------------- the maps rule
def loop_maps(lens, frames_cap):
    """the tables of a batch by a plain loop over utterances (valid input only)"""
    B = len(lens)
    fu, uo, f = [], [0], 0
    for u, n in enumerate(lens):
        fu += [u] * n
        f += n
        uo.append(f)
    fu += [B] * (frames_cap - f)
    return np.array(fu, dtype=np.int32), np.array(uo + [frames_cap], dtype=np.int32), f, sum(1 for n in lens if n > 0)


def maps_cases():
    rng = np.random.RandomState(7)
    cases = [[7, 2, 1, 9, 0, 0], [0, 0, 0], [0, 5], [3], [0], [1, 0, 1]]
    for _ in range(40):
        cases.append([int(v) for v in rng.randint(0, 12, size=rng.randint(1, 9)) * (rng.rand() < 0.8)])
    return cases


def check_inside(m, B, frames_cap, hop):
    """every index inside its buffer over the whole capacity: what hfg_bounds reads for any row g < frames_cap * rate"""
    fu, uo = m["frame_utt"], m["utt_off"]
    assert fu.shape == (frames_cap,) and uo.shape == (B + 2,) and fu.min() >= 0 and fu.max() <= B
    assert uo.min() >= 0 and uo.max() <= frames_cap and np.all(np.diff(uo) >= 0)
    f = np.arange(frames_cap)
    assert np.all(uo[fu] <= f) and np.all(f < uo[fu + 1])  # every frame lies inside the range of its owner
    assert m["live"][1] == m["live"][0] * hop and 0 <= m["live"][0] <= frames_cap


@pytest.mark.parametrize("hop", [8, 256, 384])
def test_capacity_maps_rule_against_a_loop(hop):
    from fcl_taco2_amd import hifigan

    for lens in maps_cases():
        B, total = len(lens), sum(lens)
        starts = np.concatenate([[0], np.cumsum(lens)])
        for frames_cap in sorted({max(total, 1), total + 5, total + 130}):  # live == capacity, a few dead frames, more than a tile of them
            m = hifigan.capacity_maps_rule(starts, B, frames_cap, hop)
            fu, uo, live, nz = loop_maps(lens, frames_cap)
            assert m["ok"] and m["status"] == 0
            assert np.array_equal(m["frame_utt"], fu) and np.array_equal(m["utt_off"], uo), (lens, frames_cap)
            assert m["live"].tolist() == [live, live * hop, 0, nz] and m["frame_utt"].dtype == np.int32 == m["utt_off"].dtype
            check_inside(m, B, frames_cap, hop)


@pytest.mark.parametrize("hop", [8, 256])
def test_capacity_maps_rule_refuses_instead_of_truncating(hop):
    from fcl_taco2_amd import _lib, hifigan

    B, cap = 4, 20
    dead = np.full(cap, B, dtype=np.int32)
    for starts, status, want in (([0, 7, 9, 10, 21], 0, _lib.STATUS_VOCODER_CAP),  # one frame over the capacity
                                 ([0, 7, 5, 10, 12], 0, _lib.STATUS_VOCODER_CAP),  # descending starts
                                 ([1, 7, 9, 10, 12], 0, _lib.STATUS_VOCODER_CAP),  # a non-zero first start
                                 ([0, 7, 9, 10, 12], 4, 4),                        # an incoming status: kept as it is
                                 ([0, 7, 9, 10, 21], 4, 4)):
        m = hifigan.capacity_maps_rule(starts, B, cap, hop, status=status)
        assert not m["ok"] and m["status"] == want, (starts, status)
        assert m["live"].tolist() == [0, 0, 0, 0] and np.array_equal(m["frame_utt"], dead)
        assert m["utt_off"].tolist() == [0] * (B + 1) + [cap]
        check_inside(m, B, cap, hop)
    ok = hifigan.capacity_maps_rule([0, 7, 9, 10, 20], B, cap, hop)  # exactly the capacity: live
    assert ok["ok"] and ok["live"].tolist() == [20, 20 * hop, 0, 4]


# ---------------------------------------------------------------------------------------------------------------- memory
@pytest.mark.parametrize("key", ["v1", "small"])
def test_capacity_nbytes_is_the_largest_stage_not_the_sum(key):
    """the stages share ONE set of seven row buffers: bytes per frame <= 7 x max_i(rate_i x C_i) x 4 + the small per-frame terms of the docstring"""
    from fcl_taco2_amd import hifigan

    cfg = dict(v1=R.V1, small=R.SMALL)[key]
    geo, rate = [], 1
    for i, s in enumerate(cfg["upsample_scales"]):
        rate *= s
        geo.append(rate * (cfg["channels"] >> (i + 1)))
    hop = rate
    wide = [g for i, g in enumerate(geo) if (cfg["channels"] >> (i + 1)) > 128]
    small = max(wide + [0]) * 4 + cfg["channels"] * 4 + (cfg["in_channels"] + 31) // 32 * 128 + hop * 6 + 4
    batch, frames_cap = 8, 1000
    n = hifigan.capacity_nbytes(R.plan_cfg(cfg), batch, frames_cap)
    bound = (7 * max(geo) * 4 + small) * frames_cap + 4 * (batch + 2) + 16
    unshared = 7 * sum(geo) * 4 * frames_cap
    print("%s: %d B per frame (%.0f B per sample), bound %d, unshared stage buffers alone %d" % (key, n // frames_cap, n / frames_cap / hop, bound // frames_cap,
                                                                                              unshared // frames_cap))
    assert n <= bound
    assert n < unshared if len(geo) > 1 else True
    if key == "v1":
        assert 7 * max(geo) * 4 == 229376 and n / frames_cap / hop < 1000
    assert hifigan.capacity_nbytes(R.plan_cfg(cfg), batch, 2 * frames_cap) - n == n - (4 * (batch + 2) + 16)  # linear in the capacity


def test_vocoder_graph_flag_defaults_off():
    from fcl_taco2_amd import hifigan, tts

    base = ["--model", "m", "--model-conf", "c", "--json", "j", "--vocoder-checkpoint", "v", "--outdir", "o"]
    assert tts.parse_args(base).vocoder_graph is False
    assert tts.parse_args(base + ["--vocoder-graph"]).vocoder_graph is True
    assert hifigan.HiFiGANPlan.eager_only is True and hasattr(hifigan.HiFiGANGenerator, "capacity_synth")


def test_descriptor_chain_is_one_for_both_forms():
    """hifigan.build_chain on a stub plan of CPU tensors, once with buffers of every stage's own (synthesize_packed) and once with one shared set
    (CapacitySynth): the scalars against a table written out here, the pointers against the buffers each launch has to read and write."""
    import types

    import torch

    from fcl_taco2_amd import hifigan

    t = lambda: torch.empty(8)
    unit = lambda k, d: dict(k=k, dilation=d, w1p=t(), b1=t(), w2p=t(), b2=t())
    blocks = lambda: [[unit(3, 1), unit(3, 3)], [unit(5, 1)]]  # a block of two units and a block whose one unit is first and last
    pl = types.SimpleNamespace(slope=0.1, input=dict(wp=t(), b=t(), k=7, cin=80, cout=512), stages=[
        dict(s=2, ku=4, cin=512, cout=256, wp=t(), b=t(), blocks=blocks()),  # 256 wide: the workspace tp is needed
        dict(s=4, ku=8, cin=256, cout=64, wp=t(), b=t(), blocks=blocks())])  # 64 wide: it is not
    F, fu, uo = 5, 1 << 20, 1 << 21
    f32 = lambda x: C.c_float(x).value
    #                 m_in cin  cout stride ksize padding rate_in
    want_tconv = [(5, 512, 256, 2, 4, 1, 1), (10, 256, 64, 4, 8, 2, 2)]
    #             m   c    ksize dilation rate first last cs_scale csp_slope
    want_units = [[(10, 256, 3, 1, 2, 1, 0, 0.5, 0.1), (10, 256, 3, 3, 2, 1, 1, 0.5, 0.1), (10, 256, 5, 1, 2, 0, 1, 0.5, 0.1)],
                  [(40, 64, 3, 1, 8, 1, 0, 0.5, 0.01), (40, 64, 3, 3, 8, 1, 1, 0.5, 0.01), (40, 64, 5, 1, 8, 0, 1, 0.5, 0.01)]]
    tconv_fields = ("m_in", "cin", "cout", "stride", "ksize", "padding", "rate_in")
    unit_fields = ("m", "c", "ksize", "dilation", "rate", "first", "last", "cs_scale", "csp_slope")
    scalars = []
    for shared in (False, True):
        melp, cp0, handed = t(), t(), []
        one_set = tuple(t() for _ in range(8))

        def rows_of(rows, ch):
            handed.append(one_set if shared else tuple(t() for _ in range(7)) + ((t(),) if ch not in (32, 64, 128) else (None,)))
            return handed[-1]

        a, stages, csp, rate = hifigan.build_chain(pl, F, fu, uo, melp, cp0, rows_of)
        assert (a.m, a.cin, a.cout, a.ksize, a.dilation, a.rate, a.slope) == (5, 80, 512, 7, 1, 1, f32(0.1))
        assert (a.xp, a.wp, a.bias, a.frame_utt, a.utt_off, a.y, a.yp, a.resid) == (melp.data_ptr(), pl.input["wp"].data_ptr(), pl.input["b"].data_ptr(), fu,
                                                                                      uo, None, cp0.data_ptr(), None)
        assert len(stages) == len(handed) == 2 and rate == 8 and csp is handed[-1][6]
        got, read = [], cp0  # `read`: the planes the next transposed convolution reads
        for (tc, units), st, bufs, wt, wu in zip(stages, pl.stages, handed, want_tconv, want_units):
            c, cpl, xb, cs, pa, pb, csp_, tp = [None if b is None else b.data_ptr() for b in bufs]
            assert tuple(getattr(tc, f) for f in tconv_fields) == wt and tc.slope == f32(0.1)
            assert (tc.xp, tc.wp, tc.bias, tc.frame_utt, tc.utt_off, tc.y, tc.yp) == (read.data_ptr(), st["wp"].data_ptr(), st["b"].data_ptr(), fu, uo, c, cpl)
            assert [tuple(getattr(u, f) for f in unit_fields) for u in units] == [w[:7] + (f32(w[7]), f32(w[8])) for w in wu]
            it = iter(units)
            for j, blk in enumerate(st["blocks"]):
                x, xp = c, cpl  # what the transposed convolution wrote; then what the unit before wrote
                for d, U in enumerate(blk):
                    u = next(it)
                    assert (u.x, u.xp) == (x, xp) and (u.frame_utt, u.utt_off, u.slope) == (fu, uo, f32(0.1))
                    assert (u.w1p, u.b1, u.w2p, u.b2) == tuple(U[k].data_ptr() for k in ("w1p", "b1", "w2p", "b2"))
                    if d == len(blk) - 1:
                        assert (u.x_out, u.xp_out, u.cs) == (None, None, cs) and u.csp == (csp_ if j == len(st["blocks"]) - 1 else None)
                    else:
                        assert (u.x_out, u.xp_out, u.cs, u.csp) == (xb, pa if d % 2 == 0 else pb, None, None)
                        x, xp = u.x_out, u.xp_out
                    assert u.tp == (tp if st["cout"] not in (32, 64, 128) else None) and (u.tp is None) == (st["cout"] == 64)
            got.append([tuple(getattr(tc, f) for f in tconv_fields)] + [tuple(getattr(u, f) for f in unit_fields) for u in units])
            read = bufs[6]
        scalars.append(got)
    assert scalars[0] == scalars[1]
