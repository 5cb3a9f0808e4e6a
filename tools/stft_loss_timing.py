"""Timing of the multi-resolution STFT loss on one MI355X: forward + backward of the three default resolutions

  A  torch.stft + autograd on the same device: spectra of both signals, sqrt(clamp(re^2 + im^2, 1e-7)), the two figures, (sc + mag).backward()
  B  fcl_taco2_amd.stft_loss.MultiResolutionSTFTLoss: per resolution two launches forward (frame sums, utterance sums) and two backward (frame
     gradients, gather), the [n_utt, 3] arithmetic in torch

at a training shape (`--batch` x `--clip` samples, reduction "batch") and an evaluation shape (one utterance of `--seconds` s at 22.05 kHz).  One
process; both paths are warmed up on each shape, then timed alternately: `--repeats` windows of `--iters` forward + backward passes each between
device events; the median window per pass is reported with the spread (min, max), and the two paths' results are compared on the same inputs.
Prints one JSON line.  The tool fixes no number.

    python tools/stft_loss_timing.py [--batch 8] [--clip 25600] [--seconds 10] [--repeats 7] [--iters 20]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_loss(x, y, resolutions, windows):
    """x, y [B, T] -> (sc, mag): Frobenius norms over the batch tensor, the mean of the absolute log difference, the means over the resolutions"""
    sc = mag = 0.0
    for (n_fft, hop, wl), win in zip(resolutions, windows):
        m = []
        for v in (x, y):
            S = torch.stft(v, n_fft, hop, wl, win, center=True, pad_mode="reflect", return_complex=True)
            m.append(torch.sqrt(torch.clamp(S.real ** 2 + S.imag ** 2, min=1e-7)))
        sc = sc + torch.linalg.norm(m[1] - m[0]) / torch.linalg.norm(m[1])
        mag = mag + (torch.log(m[1]) - torch.log(m[0])).abs().mean()
    return sc / len(resolutions), mag / len(resolutions)


def window_ms(step, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--clip", type=int, default=25600)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import stft_loss

    assert torch.cuda.is_available(), "stft_loss_timing.py measures on a GPU: there is no fallback"
    dev = "cuda:0"
    resolutions = list(zip(stft_loss.FFT_SIZES, stft_loss.HOP_SIZES, stft_loss.WIN_LENGTHS))
    windows = [torch.hann_window(wl, device=dev) for _, _, wl in resolutions]
    loss = stft_loss.MultiResolutionSTFTLoss(dev)
    out = dict(resolutions=resolutions, repeats=args.repeats, iters=args.iters)
    rng = np.random.RandomState(0)
    for name, (B, T) in (("training", (args.batch, args.clip)), ("evaluation", (1, int(args.seconds * 22050)))):
        y = torch.from_numpy((0.3 * rng.randn(B, T)).astype(np.float32)).to(dev)
        x = (0.8 * y + torch.from_numpy((0.05 * rng.randn(B, T)).astype(np.float32)).to(dev)).requires_grad_(True)

        def step_torch():
            x.grad = None
            sc, mag = torch_loss(x, y, resolutions, windows)
            (sc + mag).backward()
            return sc, mag

        def step_hip():
            x.grad = None
            sc, mag = loss(x, y)
            (sc + mag).backward()
            return sc, mag

        def fwd_torch():
            with torch.no_grad():
                torch_loss(x, y, resolutions, windows)

        def fwd_hip():
            with torch.no_grad():
                loss(x, y)

        # the same inputs through both paths (this is also the warm-up of every shape)
        sc_t, mag_t = step_torch()
        g_t = x.grad.clone()
        sc_h, mag_h = step_hip()
        g_h = x.grad.clone()
        for fn in (step_torch, step_hip, fwd_torch, fwd_hip):
            fn()
        torch.cuda.synchronize()
        r = dict(shape=[B, T], sc=[sc_t.item(), sc_h.item()], mag=[mag_t.item(), mag_h.item()],
                 grad_rel_diff=float((g_h - g_t).norm() / g_t.norm()))
        times = dict(torch_fwd_bwd=[], hip_fwd_bwd=[], torch_fwd=[], hip_fwd=[])
        for _ in range(args.repeats):  # alternating
            times["torch_fwd_bwd"].append(window_ms(step_torch, args.iters))
            times["hip_fwd_bwd"].append(window_ms(step_hip, args.iters))
            times["torch_fwd"].append(window_ms(fwd_torch, args.iters))
            times["hip_fwd"].append(window_ms(fwd_hip, args.iters))
        for k, v in times.items():
            r[k + "_ms"] = dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))
        r["torch_over_hip_fwd_bwd"] = r["torch_fwd_bwd_ms"]["median"] / r["hip_fwd_bwd_ms"]["median"]
        r["torch_over_hip_fwd"] = r["torch_fwd_ms"]["median"] / r["hip_fwd_ms"]["median"]
        torch.cuda.reset_peak_memory_stats()
        step_torch()
        torch.cuda.synchronize()
        r["torch_peak_bytes"] = int(torch.cuda.max_memory_allocated())
        torch.cuda.reset_peak_memory_stats()
        step_hip()
        torch.cuda.synchronize()
        r["hip_peak_bytes"] = int(torch.cuda.max_memory_allocated())
        out[name] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
