"""Kernel time of the F0 tracker beside the log-mel kernel on one MI355X: the A/B batch of tools/features_ab.py (64 utterances of about
6.5 s at 22.05 kHz, noise-like waveforms, 37 108 frames at the defaults), fx_logmel_kernel<1024> and px_yin_kernel<1024> launched alternately on maps
and buffers prepared ahead, so that one `rocprofv3 --kernel-trace --stats` run of this script holds both.  The difference function's cost does not
depend on the samples (only the few steps of the pick do), so noise serves.

Prints one JSON line: ms per launch of both kernels from event timers (every window and the median), the library's launch record, and the bytes the
tracker has to move against the HBM roofline.  The tool fixes no number.

    python tools/pitch_kernel_time.py [--batch 64] [--seconds 6.5] [--repeats 7] [--inner 20] [--frame-length 1024]
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
        fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=6.5, help="mean utterance length; lengths are drawn within +- 25 %% of it")
    ap.add_argument("--frame-length", type=int, default=1024)
    ap.add_argument("--f0-floor", type=float, default=71.0)
    ap.add_argument("--repeats", type=int, default=7, help="alternating pairs")
    ap.add_argument("--inner", type=int, default=20, help="launches per timed window")
    args = ap.parse_args()
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib, features as FX, pitch as PX

    assert torch.cuda.is_available(), "pitch_kernel_time.py measures on a GPU: there is no fallback"
    dev = torch.device("cuda:0")
    fpl = FX.FeaturePlan(dev)
    ppl = PX.PitchPlan(dev, frame_length=args.frame_length, f0_floor=args.f0_floor)
    rng = np.random.RandomState(7)
    mean = args.seconds * fpl.fs
    lens = [int(n) for n in rng.randint(int(0.75 * mean), int(1.25 * mean) + 1, size=args.batch)]
    with torch.cuda.device(dev):
        g = torch.Generator(device=dev).manual_seed(7)
        packed = (torch.rand(sum(lens), device=dev, generator=g) - 0.5) * 0.8
    mp = FX.Maps(lens, fpl.hop, dev)
    mel, en, f0 = torch.empty(mp.frames, fpl.A, device=dev), torch.empty(mp.frames, device=dev), torch.empty(mp.frames, device=dev)
    legs = {"fx_logmel_kernel<1024>": lambda: FX.launch_logmel(fpl, mp, packed, mel, en),
            "px_yin_kernel<%d>" % args.frame_length: lambda: PX.launch_yin(ppl, mp, packed, f0)}
    times = {k: [] for k in legs}
    for fn in legs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize(dev)
    for _ in range(args.repeats):
        for k, fn in legs.items():
            times[k].append(timed(fn, dev, args.inner))
    _lib.prof_enable(True)
    for fn in legs.values():
        fn()
    torch.cuda.synchronize(dev)
    rec = _lib.prof_collect()
    _lib.prof_enable(False)
    bytes_px = 4.0 * sum(lens) + 4.0 * mp.frames + 4.0 * mp.frames  # every sample once, the frame map, one word out per frame
    print(json.dumps(dict(batch=args.batch, samples=sum(lens), frames=mp.frames, frame_length=args.frame_length, tau_max=ppl.tau_max,
                          voiced_frames=int((f0 > 0).sum()), ms={k: [round(t, 4) for t in v] for k, v in times.items()},
                          median_ms={k: round(float(np.median(v)), 4) for k, v in times.items()},
                          launch_record_ms={k: round(v["ms"] / max(v["launches"], 1), 4) for k, v in rec.items() if k in legs},
                          px_bytes=int(bytes_px), px_gathered_bytes=int(4.0 * mp.frames * args.frame_length + 4.0 * mp.frames),
                          px_hbm_floor_ms=round(bytes_px / HBM_BYTES_PER_S * 1e3, 5),
                          px_fma_pairs=int(mp.frames) * (args.frame_length // 2) * 8 * ((ppl.tau_max + 2 + 7) // 8))))


if __name__ == "__main__":
    main()
