"""tests/resample_ref.py, the float64 statement of the resampling contract, against facts that need no device: unit gain, sines in the
pass band come through, tones above the output Nyquist rate are removed, the integer rules.  The bounds are about ten times what this statement gives
in float64 (the margin is for another summation order, not for the device).  The package's host-side table and refusals are checked against it."""
import numpy as np
import pytest

import resample_ref as R

RATES = [(48000, 22050), (16000, 22050), (44100, 22050), (24000, 22050)]


@pytest.mark.parametrize("pair,K", list(zip(RATES, [140, 64, 128, 70])), ids=str)
def test_table_shape_and_unit_gain(pair, K):
    L, M = R.ratio(*pair)
    assert R.half_width(L, M) == K
    c = R.table(L, M)
    assert c.shape == (L, 2 * K + 1)
    dev = np.abs(c.sum(axis=1) - 1.0).max()
    print("row sums of %r: within %.2g of 1" % (pair, dev))
    assert dev <= 1e-7
    assert c[0, K] == pytest.approx(min(1.0, L / M) * R.ROLLOFF, rel=1e-15) and c[0, 0] == 0.0  # h(0) = s rho; h(-K) = 0: |u| >= 1 there


def test_ratios_and_output_lengths():
    assert [R.ratio(*p) for p in RATES] == [(147, 320), (441, 320), (1, 2), (147, 160)] and R.ratio(22050, 16000) == (320, 441)
    for n_in in (0, 1, 2, 3, 319, 320, 321, 6000):
        assert R.out_samples(n_in, 147, 320) == n_in * 147 // 320
    assert [R.out_samples(n, 147, 320) for n in (1, 2, 3)] == [0, 0, 1] and R.out_samples(1, 441, 320) == 1
    y, a = R.resample(np.ones(2), 147, 320)
    assert len(y) == len(a) == 0


@pytest.mark.parametrize("pair", [(48000, 22050), (16000, 22050)], ids=str)
def test_sines_come_through_and_aliases_do_not(pair):
    fs_in, fs_out = pair
    L, M = R.ratio(*pair)
    K = R.half_width(L, M)
    c = R.table(L, M)
    n_in = 6000
    skip = R.edge_skip(K, L, M)
    t_in = np.arange(n_in) / fs_in
    for f in (1000.0, 0.85 * min(fs_in, fs_out) / 2):
        y, _ = R.resample(np.sin(2 * np.pi * f * t_in), L, M, c)
        assert len(y) == n_in * L // M and len(y) > 2 * skip + 100
        want = np.sin(2 * np.pi * f * np.arange(len(y)) / fs_out)
        err = np.abs(y - want)[skip:-skip].max()
        print("%r: %.0f Hz: max |y - sin| = %.2g" % (pair, f, err))
        assert err <= 1e-6
    if fs_in > fs_out:
        for k in (1.08, 1.3):
            y, _ = R.resample(np.sin(2 * np.pi * k * fs_out / 2 * t_in), L, M, c)
            left = np.abs(y)[skip:-skip].max()
            print("%r: a tone at %.2f of the output Nyquist rate leaves %.2g" % (pair, k, left))
            assert left <= 1e-6


def test_the_sum_is_the_direct_double_loop():
    """resample() (vectorised) against the contract written as two plain loops, on a short signal with both zero-filled ends in play"""
    L, M = 3, 5
    K = R.half_width(L, M)
    c = R.table(L, M)
    x = np.random.RandomState(0).randn(150)
    y, a = R.resample(x, L, M, c)
    assert len(y) == 90
    for t in (0, 1, 44, 88, 89):
        n, p = (t * M) // L, (t * M) % L
        terms = [c[p][j + K] * (x[n - j] if 0 <= n - j < len(x) else 0.0) for j in range(-K, K + 1)]
        assert y[t] == pytest.approx(sum(terms), rel=1e-12, abs=1e-15) and a[t] == pytest.approx(sum(abs(v) for v in terms), rel=1e-12)


def test_the_package_builds_the_same_table_and_refuses_what_the_kernel_does_not_cover():
    from fcl_taco2_amd import resample as RS

    assert (RS.ZEROS, RS.ROLLOFF, RS.BETA) == (R.ZEROS, R.ROLLOFF, R.BETA)
    for pair in RATES + [(22050, 16000)]:
        L, M = R.ratio(*pair)
        assert RS.ratio(*pair) == (L, M) and RS.check_rates(*pair) == (L, M, R.half_width(L, M))
        assert np.abs(RS.filter_table(L, M) - R.table(L, M)).max() <= 1e-14  # another Bessel routine: a few ulps of a value below 1
    assert [RS.out_samples(n, 147, 320) for n in (1, 2, 3, 6000)] == [0, 0, 1, 2756]
    with pytest.raises(NotImplementedError, match="22050 Hz -> 22051 Hz"):
        RS.check_rates(22050, 22051)
    with pytest.raises(NotImplementedError, match="48000 Hz -> 100 Hz"):  # 1 / 480: the filter's span does not fit LDS
        RS.check_rates(48000, 100)
    with pytest.raises(ValueError, match="positive"):
        RS.check_rates(0, 22050)
    with pytest.raises(RS._lib.FclError, match="GPU"):
        RS.ResamplePlan("cpu", 16000, 22050)


def test_ctypes_mirror_of_the_argument_struct_matches_the_header(tmp_path):
    """_lib.Resample is laid out like fcl_rs_t: a C program that includes the header prints sizeof and every field's offset"""
    import ctypes as C
    import subprocess

    from conftest import ROOT
    from fcl_taco2_amd import _lib

    names = [n for n, _ in _lib.Resample._fields_]
    body = ['#include <stdio.h>', '#include <stddef.h>', '#include "fcl_hip.h"', "int main(void) {", '  printf("%zu", sizeof(fcl_rs_t));']
    body += ['  printf(" %%zu", offsetof(fcl_rs_t, %s));' % n for n in names] + ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(body))
    subprocess.run(["gcc", "-I", "%s/include" % ROOT, str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(_lib.Resample)] + [getattr(_lib.Resample, n).offset for n in names]


def test_entry_point_validates_arguments_without_a_gpu():
    """fcl_rs_resample_fwd returns before any HIP call: -1 for a null pointer, -2 for L < 1, M < 1 or a negative count, 0 for an empty batch"""
    import ctypes as C

    from fcl_taco2_amd import _lib

    lib = _lib.load()
    assert lib.fcl_rs_resample_fwd(None, None) == -1
    a = _lib.Resample()
    a.l, a.m, a.k, a.n_utt, a.max_out, a.samples_in, a.samples_out = 147, 320, 140, 1, 10, 30, 10
    assert lib.fcl_rs_resample_fwd(C.byref(a), None) == -1 and b"null" in lib.fcl_last_error()
    for f in ("x", "smp_off_in", "smp_off_out", "table", "y"):
        setattr(a, f, 256)
    for field, bad in (("l", 0), ("m", 0), ("n_utt", -1), ("samples_in", -1), ("samples_out", -5), ("max_out", -1), ("k", 0)):
        good = getattr(a, field)
        setattr(a, field, bad)
        assert lib.fcl_rs_resample_fwd(C.byref(a), None) == -2, field
        setattr(a, field, good)
    a.l, a.m = 294, 640
    assert lib.fcl_rs_resample_fwd(C.byref(a), None) == -2 and b"lowest terms" in lib.fcl_last_error()
    a.l, a.m, a.k = 1, 480, 30720
    assert lib.fcl_rs_resample_fwd(C.byref(a), None) == -2 and b"supported range" in lib.fcl_last_error()
    a.l, a.m, a.k, a.n_utt = 147, 320, 140, 0
    assert lib.fcl_rs_resample_fwd(C.byref(a), None) == 0
