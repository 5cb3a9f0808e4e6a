"""Timing of the mel-spectrogram L1 loss on one MI355X: forward + backward of the default resolution (n_fft 1024, hop 256, 80 mels)

  A  torch.stft + matmul + log10 + autograd on the same device: spectra of both signals, sqrt(clamp(re^2 + im^2, 1e-10)), the dense
     [bins, n_mels] projection, log10(clamp(., 1e-10)), F.l1_loss, backward()
  B  fcl_taco2_amd.mel_loss.MelSpectrogramLoss: two launches forward (frame sums, utterance sums) and two backward (frame gradients, gather), the
     [n_utt] arithmetic in torch

at the training shape (`--batch` x `--clip` samples, reduction "batch") and an evaluation shape (one utterance of `--seconds` s at 22.05 kHz).  One
process; both paths are warmed up on each shape, then timed alternately: `--repeats` windows of `--iters` forward + backward passes each between
device events; the median window per pass is reported with the spread (min, max) and the peak memory of one pass, and the two float32 paths'
results are compared on the same inputs.  Prints one JSON line.  The tool fixes no number.

    python tools/mel_loss_timing.py [--batch 8] [--clip 25600] [--seconds 10] [--repeats 7] [--iters 20]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FLOOR = 1e-10


def torch_loss(x, y, resolutions, windows, bases):
    """x, y [B, T] -> F.l1_loss of the two log10 mel tensors, the mean over the resolutions"""
    out = 0.0
    for (n_fft, hop, wl), win, Bt in zip(resolutions, windows, bases):
        l = []
        for v in (x, y):
            S = torch.stft(v, n_fft, hop, wl, win, center=True, pad_mode="reflect", return_complex=True)
            m = torch.sqrt(torch.clamp(S.real ** 2 + S.imag ** 2, min=FLOOR))
            l.append(torch.log10(torch.clamp(m.transpose(1, 2) @ Bt, min=FLOOR)))
        out = out + torch.nn.functional.l1_loss(l[0], l[1])
    return out / len(resolutions)


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
    from fcl_taco2_amd import mel_loss

    assert torch.cuda.is_available(), "mel_loss_timing.py measures on a GPU: there is no fallback"
    dev = "cuda:0"
    loss = mel_loss.MelSpectrogramLoss(dev)
    resolutions = loss.plan.configs
    windows = [torch.hann_window(wl, device=dev) for _, _, wl in resolutions]
    bases = [torch.from_numpy(np.ascontiguousarray(rs.B.T, dtype=np.float32)).to(dev) for rs in loss.plan.resolutions]
    out = dict(resolutions=resolutions, n_mels=[rs.n_mels for rs in loss.plan.resolutions], repeats=args.repeats, iters=args.iters)
    rng = np.random.RandomState(0)
    for name, (B, T) in (("training", (args.batch, args.clip)), ("evaluation", (1, int(args.seconds * 22050)))):
        y = torch.from_numpy((0.3 * rng.randn(B, T)).astype(np.float32)).to(dev)
        x = (0.8 * y + torch.from_numpy((0.05 * rng.randn(B, T)).astype(np.float32)).to(dev)).requires_grad_(True)

        def step_torch():
            x.grad = None
            v = torch_loss(x, y, resolutions, windows, bases)
            v.backward()
            return v

        def step_hip():
            x.grad = None
            v = loss(x, y)
            v.backward()
            return v

        def fwd_torch():
            with torch.no_grad():
                torch_loss(x, y, resolutions, windows, bases)

        def fwd_hip():
            with torch.no_grad():
                loss(x, y)

        # the same inputs through both paths (this is also the warm-up of every shape)
        v_t = step_torch()
        g_t = x.grad.clone()
        v_h = step_hip()
        g_h = x.grad.clone()
        for fn in (step_torch, step_hip, fwd_torch, fwd_hip):
            fn()
        torch.cuda.synchronize()
        r = dict(shape=[B, T], loss=[v_t.item(), v_h.item()], grad_rel_diff=float((g_h - g_t).norm() / g_t.norm()))
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
        base = int(torch.cuda.memory_allocated())
        torch.cuda.reset_peak_memory_stats()
        step_torch()
        torch.cuda.synchronize()
        r["torch_peak_bytes"] = int(torch.cuda.max_memory_allocated()) - base
        torch.cuda.reset_peak_memory_stats()
        step_hip()
        torch.cuda.synchronize()
        r["hip_peak_bytes"] = int(torch.cuda.max_memory_allocated()) - base
        out[name] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
