"""Band-limited resampling on the HIP path: a packed batch of waveforms at fs_in -> the same batch at fs_out (csrc/resample.hip).

The reference resamples a wav whose rate is not the analysis rate with `resampy.resample` (preprocess.py lines 37-39).  This is the same filter, a
Kaiser-windowed sinc with 64 zero crossings, roll-off 0.9475937167399596 and beta 14.769656459379492 (the published parameters of that library's
default filter), evaluated exactly at the L phases of the rational ratio fs_out / fs_in = L / M instead of interpolated in a table.  The contract is
stated in include/fcl_hip.h "Resampling" and restated in float64 numpy in tests/resample_ref.py; `resampy` is not available here, so parity with it
stays unpinned (DESIGN §6g names what a comparison would have to confirm).

An utterance of n_in samples gives n_out = (n_in L) // M samples.  Equal rates are the identity and launch nothing.  No CPU fallback."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib, ops

ZEROS, ROLLOFF, BETA = 64, 0.9475937167399596, 14.769656459379492
L_MAX, TABLE_BYTES_MAX, SPAN_CAP = 1024, 4 << 20, 12288  # SPAN_CAP: the floats of LDS a tile's input span may take (csrc/resample.hip)


def ratio(fs_in, fs_out):
    """(L, M): fs_out / fs_in = L / M in lowest terms"""
    fs_in, fs_out = int(fs_in), int(fs_out)
    if fs_in < 1 or fs_out < 1:
        raise ValueError("fcl-taco2_amd: resample: sampling rates must be positive (got %d -> %d)" % (fs_in, fs_out))
    g = math.gcd(fs_in, fs_out)
    return fs_out // g, fs_in // g


def half_width(L, M):
    """K = ceil(Z / s), s = min(1, L / M), in integers"""
    return ZEROS if M <= L else -((-ZEROS * M) // L)


def out_samples(n_in, L, M):
    """samples of the resampled utterance: (n_in L) // M"""
    return (int(n_in) * int(L)) // int(M)


def filter_table(L, M):
    """c [L][2 K + 1] float64: c[p][j + K] = h(j + p / L), h(tau) = s rho sinc(s rho tau) I0(beta sqrt(1 - u^2)) / I0(beta), u = s tau / Z, 0 for |u| >= 1"""
    K = half_width(L, M)
    s = min(1.0, L / M)
    tau = np.arange(-K, K + 1, dtype=np.float64)[None, :] + np.arange(L, dtype=np.float64)[:, None] / L
    u = s * tau / ZEROS
    win = np.i0(BETA * np.sqrt(np.maximum(1.0 - u * u, 0.0))) / np.i0(BETA)
    return np.where(np.abs(u) < 1.0, s * ROLLOFF * np.sinc(s * ROLLOFF * tau) * win, 0.0)


def check_rates(fs_in, fs_out):
    """What the kernel covers: L <= 1024, a table of at most 4 MB and a filter whose span fits LDS (ratios down to 1 / 64).  Anything else is
    refused naming both rates, before any device call.  -> (L, M, K)"""
    L, M = ratio(fs_in, fs_out)
    K = half_width(L, M)
    if L > L_MAX or L * (2 * K + 1) * 4 > TABLE_BYTES_MAX or 64 * M > (SPAN_CAP - 2 * K - 2) * L:
        raise NotImplementedError("fcl-taco2_amd: resample: %d Hz -> %d Hz (L / M = %d / %d, %d taps per phase) is not supported on the HIP path: L <= %d, "
                                  "a table of at most %d MB and 64 M / L + 2 K + 2 <= %d are" % (fs_in, fs_out, L, M, 2 * K + 1, L_MAX, TABLE_BYTES_MAX >> 20, SPAN_CAP))
    return L, M, K


class ResamplePlan(object):
    """fs_in -> fs_out: L, M, K, the float64 `table` [L][2 K + 1] and its float32 transpose [2 K + 1][L] on the device (`table_d`).  Equal rates:
    the identity, no table."""

    def __init__(self, device, fs_in, fs_out):
        self.fs_in, self.fs_out = int(fs_in), int(fs_out)
        self.L, self.M, self.K = check_rates(fs_in, fs_out)
        self.identity = self.fs_in == self.fs_out
        if not str(device).startswith("cuda"):
            raise _lib.FclError("fcl-taco2_amd: ResamplePlan needs a GPU device (no CPU fallback)")
        self.device = torch.device(device)
        self.table, self.table_d = None, None
        if not self.identity:
            self.table = filter_table(self.L, self.M)
            with torch.cuda.device(self.device):
                self.table_d = torch.from_numpy(np.ascontiguousarray(self.table.T, dtype=np.float32)).to(self.device)

    def out_samples(self, n_in):
        return out_samples(n_in, self.L, self.M)


def offsets(lens, dev):
    """[n_utt + 1] int32 exclusive sums on the device"""
    return torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)).to(dev)


def launch_resample(pl, x, smp_off_in, smp_off_out, y, n_utt, samples_in, samples_out, max_out):
    """one launch on caller-owned buffers (the tests surround them with guard zones): x [samples_in] -> y [samples_out]"""
    a = _lib.Resample()
    a.samples_in, a.samples_out, a.l, a.m, a.k, a.n_utt, a.max_out = int(samples_in), int(samples_out), pl.L, pl.M, pl.K, int(n_utt), int(max_out)
    a.x, a.smp_off_in, a.smp_off_out, a.table, a.y = x.data_ptr(), smp_off_in.data_ptr(), smp_off_out.data_ptr(), pl.table_d.data_ptr(), y.data_ptr()
    _lib.check(_lib.load().fcl_rs_resample_fwd(C.byref(a), ops._stream()))


class Resampler(object):
    """Resampling on a ResamplePlan."""

    def __init__(self, plan):
        self.plan = plan

    def resample_packed(self, x, lens, ids=None):
        """x: the utterances' samples back to back ([sum n_in] float32, device tensor or array), lens: samples per utterance ->
        (y [sum n_out] float32 on the device, out_lens): ONE launch; none at equal rates."""
        pl, dev = self.plan, self.plan.device
        lens = [int(n) for n in lens]
        with torch.cuda.device(dev):
            x = torch.as_tensor(x).to(device=dev, dtype=torch.float32).contiguous().reshape(-1)
            if x.numel() != sum(lens) or any(n < 0 for n in lens):
                raise _lib.FclError("fcl-taco2_amd: resample: the packed waveform has %d samples, lens sum to %d" % (x.numel(), sum(lens)))
            if pl.identity:
                return x, lens
            out_lens = [pl.out_samples(n) for n in lens]
            if sum(lens) >= 2 ** 31 - 1 or sum(out_lens) >= 2 ** 31 - 1 or len(lens) > 65535:
                raise _lib.FclError("fcl-taco2_amd: more than 2^31 samples or 65535 utterances in one resampling batch (%d Hz -> %d Hz)" % (pl.fs_in, pl.fs_out))
            y = torch.empty(sum(out_lens), device=dev, dtype=torch.float32)
            if lens and max(out_lens) > 0:
                launch_resample(pl, x, offsets(lens, dev), offsets(out_lens, dev), y, len(lens), sum(lens), sum(out_lens), max(out_lens))
        return y, out_lens


class ResamplerCache(object):
    """Resamplers to one output rate by input rate, built on first use (extract_features.extract's `resampler_for`)"""

    def __init__(self, device, fs_out):
        self.device, self.fs_out, self.by_rate = device, int(fs_out), {}

    def __call__(self, fs_in):
        if fs_in not in self.by_rate:
            self.by_rate[fs_in] = Resampler(ResamplePlan(self.device, fs_in, self.fs_out))
        return self.by_rate[fs_in]
