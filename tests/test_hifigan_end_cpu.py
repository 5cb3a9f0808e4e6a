"""The float64 statement of the HiFi-GAN generator's output end (tests/hfge_ref.py) checked without a device: against F.leaky_relu +
F.conv1d + tanh under float64 autograd, its bounds against float32 evaluations of exactly the arrays tests/test_gpu_hifigan_end.py runs, its mutants;
and the C entries' argument checks, the struct layout and the module's refusal of an unknown output_end."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hfge_ref as E
from conftest import ROOT

LENS = list(E.LENS)
F64, F32 = np.float64, np.float32


def case64(c, cout, k):
    x, w, b, dwav = E.end_case(c, cout, k)
    return tuple(np.asarray(v, F64) for v in (x, w, b, dwav)) + (E.given_wav(x, w, b, LENS).astype(F64),)


@pytest.mark.parametrize("c,cout,k", E.CELLS)
def test_statement_agrees_with_torch_under_float64_autograd(c, cout, k):
    x, w, b, dwav, _ = case64(c, cout, k)
    xt, wt, bt = (torch.tensor(v, requires_grad=True) for v in (x, w, b))
    outs = [torch.tanh(F.conv1d(F.leaky_relu(xx.T.unsqueeze(0), E.OUT_SLOPE), wt, bt, padding=(k - 1) // 2))[0].T for xx in torch.split(xt, LENS)]
    wav_t = torch.cat(outs)
    (wav_t * torch.tensor(dwav)).sum().backward()
    wav, _ = E.end_fwd(x, w, b, LENS)
    dx, _, unsure = E.end_dx(x, w, wav, dwav, LENS)
    dW, db, _, _ = E.end_dw(x, wav, dwav, k, LENS)
    assert unsure == 0.0
    for got, want in ((wav, wav_t.detach()), (dx, xt.grad), (dW, wt.grad), (db, bt.grad)):
        assert np.abs(got - want.numpy()).max() < 1e-12


@pytest.mark.parametrize("c,cout,k", E.CELLS)
def test_float32_evaluation_stays_inside_every_bound(c, cout, k):
    x, w, b, dwav, given = case64(c, cout, k)
    wav, e_wav = E.end_fwd(x, w, b, LENS)
    assert E.share(E.end_fwd(x, w, b, LENS, dt=F32)[0] - wav, e_wav) <= 1.0
    dx, e_dx, _ = E.end_dx(x, w, given, dwav, LENS)
    assert E.share(E.end_dx(x, w, given, dwav, LENS, dt=F32)[0] - dx, e_dx) <= 1.0
    dW, db, e_dW, e_db = E.end_dw(x, given, dwav, k, LENS)
    g32 = E.end_dw(x, given, dwav, k, LENS, dt=F32)
    assert E.share(g32[0] - dW, e_dW) <= 1.0 and E.share(g32[1] - db, e_db) <= 1.0


# which outputs a mutant must push outside their bound
HITS = dict(taps_not_reversed=("dx",), mask_dropped=("dx",), tanh_prime_dropped=("dx", "dW", "db"), tanh_prime_abs=("dx", "dW"),
            tap_across_edge=("wav", "dx", "dW"), missing_bias_gradient=("db",), stage_slope=("wav", "dx", "dW"))


def outputs(x, w, b, dwav, given, k, mutant=None):
    wav, e_wav = E.end_fwd(x, w, b, LENS, mutant=mutant)
    dx, e_dx, _ = E.end_dx(x, w, given, dwav, LENS, mutant=mutant)
    dW, db, e_dW, e_db = E.end_dw(x, given, dwav, k, LENS, mutant=mutant)
    return dict(wav=(wav, e_wav), dx=(dx, e_dx), dW=(dW, e_dW), db=(db, e_db))


@pytest.mark.parametrize("mutant", E.MUTANTS)
def test_every_mutant_leaves_its_bound(mutant):
    assert set(HITS) == set(E.MUTANTS)
    for c, cout, k in E.CELLS:
        x, w, b, dwav, given = case64(c, cout, k)
        ref, mut = outputs(x, w, b, dwav, given, k), outputs(x, w, b, dwav, given, k, mutant)
        for name in HITS[mutant]:
            assert E.share(mut[name][0] - ref[name][0], ref[name][1]) > 1.0, (mutant, name, c, cout, k)


def test_the_tanh_constant_is_twice_the_recorded_observation():
    assert E.E_TANH == 2 * E.E_TANH_OBSERVED and 0 < E.E_TANH_OBSERVED < 4


def test_sweep_case_is_one_product_over_the_whole_range():
    x, w, b, pre, e_pre = E.sweep_case(1001)
    assert np.count_nonzero(w) == 1 and not b.any() and pre.min() < -8.99 and pre.max() > 8.99
    full, _ = E.end_pre(x.astype(F64), w.astype(F64), b.astype(F64), [len(x)])
    assert np.array_equal(full, pre)


def test_c_entries_validate_without_a_gpu(tmp_path):
    import __graft_entry__ as ge

    ge.build()
    from fcl_taco2_amd import _lib

    lib = _lib.load()
    entries = fwd, dx, dw = lib.fcl_hfe_fwd, lib.fcl_hfe_dx, lib.fcl_hfe_dw
    for f in entries:
        assert f(None, None) == -1 and b"null" in lib.fcl_last_error()

    def filled(**kw):
        a = _lib.HfeEnd()
        a.rows, a.cin, a.cout, a.ksize, a.slope = 100, 64, 2, 7, 0.01
        for n, t in _lib.HfeEnd._fields_:
            if t is C.c_void_p:
                setattr(a, n, 256)
        a.workspace_bytes = 1 << 30
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for f in entries:
        for bad in (dict(cin=24), dict(cin=0), dict(cin=272)):
            assert f(C.byref(filled(**bad)), None) == -2 and b"multiple of 16" in lib.fcl_last_error(), bad
        for bad in (dict(cout=0), dict(cout=5)):
            assert f(C.byref(filled(**bad)), None) == -2 and b"cout" in lib.fcl_last_error(), bad
        for k in (1, 2, 4, 9, 13):
            assert f(C.byref(filled(ksize=k)), None) == -2 and b"kernel size" in lib.fcl_last_error()
        assert f(C.byref(filled(rows=0)), None) == -2 and f(C.byref(filled(rows=2 ** 31)), None) == -2
        assert f(C.byref(filled(slope=1.0)), None) == -1 and f(C.byref(filled(slope=-0.1)), None) == -1 and b"slope" in lib.fcl_last_error()
        assert f(C.byref(filled(seg_lo=None)), None) == -1 and f(C.byref(filled(seg_hi=None)), None) == -1
    for f, names, aligned in ((fwd, ("x", "w", "bias", "wav"), ("x", "w")), (dx, ("x", "w", "wav", "dwav", "dx"), ("x", "w", "dx")),
                              (dw, ("x", "wav", "dwav", "dw", "db", "workspace"), ("x", "workspace"))):
        for n in names:
            assert f(C.byref(filled(**{n: None})), None) == -1, n
        for n in aligned:
            assert f(C.byref(filled(**{n: 260})), None) == -3 and b"16-byte" in lib.fcl_last_error(), n
    need = lib.fcl_hfe_workspace_bytes(100, 64, 2, 7)
    assert need == 1 * (7 * 64 + 1) * 2 * 4 and lib.fcl_hfe_workspace_bytes(1025, 16, 1, 3) == 2 * (3 * 16 + 1) * 4
    assert lib.fcl_hfe_workspace_bytes(0, 64, 2, 7) == 0
    assert dw(C.byref(filled(workspace_bytes=need - 4)), None) == -5 and b"workspace" in lib.fcl_last_error()
    # the ctypes mirror is laid out like the header's struct
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fcl_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(fcl_hfe_t), '
                   'offsetof(fcl_hfe_t, slope), offsetof(fcl_hfe_t, seg_lo), offsetof(fcl_hfe_t, dwav), offsetof(fcl_hfe_t, workspace_bytes)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    A = _lib.HfeEnd
    assert out == [C.sizeof(A), A.slope.offset, A.seg_lo.offset, A.dwav.offset, A.workspace_bytes.offset]


def test_unknown_output_end_is_refused_by_name():
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import hifigan_generator as G

    gen = G.TrainableHiFiGANGenerator(in_channels=16, channels=64, upsample_scales=(2,), upsample_kernel_sizes=(4,), resblock_kernel_sizes=(3,),
                                      resblock_dilations=((1,),))
    with pytest.raises(ValueError, match="output_end='x'"):
        gen(torch.zeros(1, 16, 4), output_end="x")
    assert G.OUTPUT_ENDS == ("torch", "hip") and G.END_FWD == "hfe_fwd_kernel" and G.END_DW == ("hfe_dw_kernel", "hfe_dw_reduce_kernel")
    w = torch.randn(2, 32, 7)
    assert torch.equal(G.pack_end(w).permute(1, 2, 0), w)
