"""A/B of the two ways to compute log-mel and energy features on one MI355X: 64 utterances of about 6.5 s at 22.05 kHz (noise-like
waveforms), the default analysis (n_fft 1024, hop 256, 80 mels).

  A  the same analysis on torch.stft (torch-ROCm's FFT library) on the zero-padded [64, L_max] batch, a matmul with the dense filterbank, log10 and
     the 2-norm over the bins -- which also computes the padding's frames and writes the complex spectrum and the magnitudes to HBM
  B  FeatureExtractor.extract_packed on the packed samples (csrc/features.hip: one launch) -- the call a driver makes, so it includes building the
     batch's maps on the host, three small uploads and the output allocations
  B_launch_only  the same launch on maps and buffers prepared ahead of time, as leg A's inputs are: the kernel and its launch alone

One process, alternating legs, event timers, a synchronise at each batch end.  Prints one JSON line: ms per batch of both legs (every run and the
median), the bytes leg B has to move against the HBM roofline, the largest difference of the two legs on the longest utterance (which has no padding in
leg A), and with --prof the kernel's ms from the library's launch record.  --skip-torch: leg B only (a kernel-trace run).  The tool fixes no number.

    python tools/features_ab.py [--batch 64] [--seconds 6.5] [--repeats 7] [--inner 20] [--prof] [--skip-torch]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12  # MI355X: 8 TB/s peak


def timed(fn, dev, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        out = fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) / inner, out


def torch_features(x, window, B_t, n_fft, hop):
    """x [batch, L_max] zero-padded -> (log-mel [batch, T_max, n_mels], energy [batch, T_max])"""
    S = torch.stft(x, n_fft, hop, window=window, center=True, pad_mode="reflect", return_complex=True).abs().transpose(1, 2)
    return torch.log10(torch.clamp(S @ B_t, min=1e-10)), torch.linalg.vector_norm(S, dim=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=6.5, help="mean utterance length; lengths are drawn within +- 25 %% of it")
    ap.add_argument("--n-fft", type=int, default=1024)
    ap.add_argument("--hop", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=7, help="alternating pairs")
    ap.add_argument("--inner", type=int, default=20, help="calls per timed window")
    ap.add_argument("--skip-torch", action="store_true", help="leg B only (a kernel-trace run)")
    ap.add_argument("--prof", action="store_true", help="also one profiled pass of leg B: the kernel's ms from the library's launch record")
    args = ap.parse_args()
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib, features as FX

    assert torch.cuda.is_available(), "features_ab.py measures on a GPU: there is no fallback"
    dev = torch.device("cuda:0")
    pl = FX.FeaturePlan(dev, n_fft=args.n_fft, hop=args.hop)
    fx = FX.FeatureExtractor(pl)
    rng = np.random.RandomState(7)
    mean = args.seconds * pl.fs
    lens = [int(n) for n in rng.randint(int(0.75 * mean), int(1.25 * mean) + 1, size=args.batch)]
    frames = sum(fx.frames_of(n) for n in lens)
    with torch.cuda.device(dev):
        g = torch.Generator(device=dev).manual_seed(7)
        packed = (torch.rand(sum(lens), device=dev, generator=g) - 0.5) * 0.8
    legs = {}
    if not args.skip_torch:
        padded = torch.zeros(args.batch, max(lens), device=dev)
        off = np.concatenate([[0], np.cumsum(lens)])
        for i, n in enumerate(lens):
            padded[i, :n] = packed[off[i] : off[i + 1]]
        B_t = torch.from_numpy(np.ascontiguousarray(pl.B.T, dtype=np.float32)).to(dev)
        legs["A_torch_stft_padded"] = lambda: torch_features(padded, pl.window_d, B_t, args.n_fft, args.hop)
    legs["B_hip"] = lambda: fx.extract_packed(packed, lens)
    mp = FX.Maps(lens, args.hop, dev)
    mel_b, en_b = torch.empty(mp.frames, pl.A, device=dev), torch.empty(mp.frames, device=dev)
    legs["B_launch_only"] = lambda: FX.launch_logmel(pl, mp, packed, mel_b, en_b)
    times = {k: [] for k in legs}
    with torch.no_grad():
        for k, fn in legs.items():  # warm-up: code objects, allocator, FFT plans
            for _ in range(3):
                fn()
            torch.cuda.synchronize(dev)
        for _ in range(args.repeats):
            for k, fn in legs.items():  # alternating legs
                times[k].append(timed(fn, dev, args.inner)[0])
    # what leg B has to move at least: every sample once from HBM, the frame maps, and per frame n_mels + 1 words out.  ASSUMED, not measured: the
    # n_fft / hop re-reads of neighbouring frames all hit in cache (B_hip_gathered_bytes counts them in full); the window, twiddle and filter
    # tables (a few KB, cache resident) are left out
    bytes_b = 4.0 * sum(lens) + 4.0 * frames + 4.0 * frames * (pl.A + 1)
    out = dict(batch=args.batch, samples=sum(lens), frames=frames, audio_s=sum(lens) / float(pl.fs), n_fft=args.n_fft, hop=args.hop,
               ms={k: [round(t, 4) for t in v] for k, v in times.items()}, median_ms={k: round(float(np.median(v)), 4) for k, v in times.items()},
               B_hip_bytes=int(bytes_b), B_hip_gathered_bytes=int(4.0 * frames * args.n_fft + 4.0 * frames * (pl.A + 1)),
               B_hip_hbm_floor_ms=round(bytes_b / HBM_BYTES_PER_S * 1e3, 5))
    if not args.skip_torch:
        i = int(np.argmax(lens))
        with torch.no_grad():
            (ma, ea), (mb, eb, fl) = legs["A_torch_stft_padded"](), legs["B_hip"]()
        fo = np.concatenate([[0], np.cumsum(fl)])
        ma, ea, mb, eb = ma[i, : fl[i]], ea[i, : fl[i]], mb[fo[i] : fo[i + 1]], eb[fo[i] : fo[i + 1]]
        out["max_abs_diff_longest_utterance"] = dict(logmel=float((ma - mb).abs().max()), energy_rel=float(((ea - eb).abs() / eb).max()))
    if args.prof:
        _lib.prof_enable(True)
        legs["B_hip"]()
        torch.cuda.synchronize(dev)
        rec = _lib.prof_collect()
        _lib.prof_enable(False)
        out["kernels"] = {k: dict(launches=v["launches"], ms=round(v["ms"], 4)) for k, v in rec.items() if k.startswith("fx_")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
