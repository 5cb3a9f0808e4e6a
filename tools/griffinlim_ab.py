"""A/B of the two ways to run Griffin-Lim on one MI355X: 64 utterances of 420 - 720 frames (the batch of DESIGN 6b), magnitudes of noise-like
spectra, the same random initial phase in both legs.

  A  the same iteration on torch.stft / torch.istft (torch-ROCm's FFT library) on the zero-padded [64, F, T_max] batch
  B  GriffinLim.iterate on the packed rows (csrc/griffinlim.hip: three launches per iteration)
  (for orientation) the Parallel WaveGAN generator on the same number of frames

One process, alternating legs, event timers, a synchronise at each batch end.  Prints one JSON line: ms per batch, RTF, per-kernel ms of leg B with
--prof, and the spectral convergence both legs reach on the longest utterance (which has no padding in leg A).  The tool fixes no number.

    python tools/griffinlim_ab.py [--batch 64] [--frames-lo 420] [--frames-hi 720] [--iters 64] [--repeats 5] [--prof] [--skip-torch]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b), out


def torch_griffin_lim(S, P, window, n_fft, hop, n_iter, momentum):
    """S [B, F, T] magnitudes, P [B, F, T] complex phases -> [B, hop (T - 1)]"""
    alpha, length = momentum / (1.0 + momentum), hop * (S.shape[2] - 1)
    c_prev = torch.zeros_like(P)
    for _ in range(n_iter):
        y = torch.istft(S * P, n_fft, hop, window=window, center=True, length=length)
        c = torch.stft(y, n_fft, hop, window=window, center=True, pad_mode="reflect", return_complex=True)
        a = c - alpha * c_prev
        P = a / (a.abs() + 1e-16)
        c_prev = c
    return torch.istft(S * P, n_fft, hop, window=window, center=True, length=length)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames-lo", type=int, default=420)
    ap.add_argument("--frames-hi", type=int, default=720)
    ap.add_argument("--iters", type=int, default=64)
    ap.add_argument("--momentum", type=float, default=0.99)
    ap.add_argument("--n-fft", type=int, default=1024)
    ap.add_argument("--hop", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-torch", action="store_true", help="leg B only (a kernel-trace run)")
    ap.add_argument("--prof", action="store_true", help="also one profiled pass of leg B: per-kernel ms from the library's launch record")
    args = ap.parse_args()
    import fcl_taco2_amd  # noqa: F401
    import griffinlim_ref as R
    from fcl_taco2_amd import _lib, griffinlim as GL, vocoder

    dev = torch.device("cuda:0")
    rng = np.random.RandomState(7)
    lens = [int(n) for n in rng.randint(args.frames_lo, args.frames_hi + 1, size=args.batch)]
    pl = GL.GriffinLimPlan(dev, n_fft=args.n_fft, hop=args.hop, n_iter=args.iters, momentum=args.momentum)
    gen, mp = GL.GriffinLim(pl), GL.Maps(lens, dev)
    frames, bins, t_max = sum(lens), pl.bins, max(lens)
    with torch.cuda.device(dev):
        g = torch.Generator(device=dev).manual_seed(7)
        S = torch.rand(frames, bins, device=dev, generator=g) ** 2 + 1e-3
        P0 = torch.polar(torch.ones(frames, bins, device=dev), 2 * np.pi * torch.rand(frames, bins, device=dev, generator=g))
    legs = {}
    if not args.skip_torch:
        Sp, Pp = torch.zeros(args.batch, bins, t_max, device=dev), torch.zeros(args.batch, bins, t_max, device=dev, dtype=torch.complex64)
        for i in range(args.batch):
            lo, hi = int(mp.frame_off[i]), int(mp.frame_off[i + 1])
            Sp[i, :, : lens[i]], Pp[i, :, : lens[i]] = S[lo:hi].T, P0[lo:hi].T
        win = pl.window_d
        legs["A_torch_stft_padded"] = lambda: torch_griffin_lim(Sp, Pp, win, args.n_fft, args.hop, args.iters, args.momentum)
    legs["B_hip"] = lambda: gen.iterate(mp, S, P0.clone())
    if not args.skip_torch:
        import helpers as H

        pwg = vocoder.ParallelWaveGANGenerator(vocoder.PWGPlan(H.pwg_random_state_dict(np.random.RandomState(1), None, 1.0), dev))
        mel = torch.randn(frames, 80, device=dev, generator=g)
        legs["PWG_same_frames"] = lambda: pwg.synthesize_packed(mel, lens, seed=1)
    times = {k: [] for k in legs}
    with torch.no_grad():
        for k, fn in legs.items():  # warm-up: one-time setup, allocator, FFT plans
            fn()
            torch.cuda.synchronize(dev)
        for _ in range(args.repeats):
            for k, fn in legs.items():  # alternating legs
                times[k].append(timed(fn, dev)[0])
    samples = args.hop * (frames - args.batch)
    out = dict(batch=args.batch, frames=frames, samples=samples, iters=args.iters, n_fft=args.n_fft, hop=args.hop, audio_s=samples / float(pl.fs),
               ms={k: [round(t, 2) for t in v] for k, v in times.items()}, median_ms={k: round(float(np.median(v)), 2) for k, v in times.items()})
    out["rtf"] = {k: round(v / 1000.0 / out["audio_s"], 6) for k, v in out["median_ms"].items()}
    # what both legs reach on the longest utterance (float64 measure of tests/griffinlim_ref.py)
    i = int(np.argmax(lens))
    lo, hi = int(mp.frame_off[i]), int(mp.frame_off[i + 1])
    s64, w64 = S[lo:hi].cpu().numpy().astype(np.float64), pl.window.astype(np.float32).astype(np.float64)
    so = (lo - i) * args.hop
    with torch.no_grad():
        yb = legs["B_hip"]()[so : so + args.hop * (lens[i] - 1)].cpu().numpy().astype(np.float64)
        out["convergence"] = dict(B_hip=round(R.spectral_convergence(yb, s64, w64, args.hop), 5))
        if not args.skip_torch:
            ya = legs["A_torch_stft_padded"]()[i].cpu().numpy().astype(np.float64)
            out["convergence"]["A_torch_stft_padded"] = round(R.spectral_convergence(ya, s64, w64, args.hop), 5)
    if args.prof:
        _lib.prof_enable(True)
        legs["B_hip"]()
        torch.cuda.synchronize(dev)
        rec = _lib.prof_collect()
        _lib.prof_enable(False)
        out["kernels"] = {k: dict(launches=v["launches"], ms=round(v["ms"], 3)) for k, v in rec.items() if k.startswith("gl_")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
