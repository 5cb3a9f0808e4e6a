"""Kernel time of the probabilistic YIN launches beside px_yin_kernel on one MI355X: the timing batch of tools/pitch_kernel_time.py (64
utterances of about 6.5 s at 22.05 kHz, 37 108 frames at the defaults), here a 150 Hz tone of six harmonics under noise so that frames have
candidates.  px_yin_kernel<1024> (writing d'), pyin_obs_kernel and pyin_viterbi_kernel are launched on maps and buffers prepared ahead.

Prints one JSON line: ms per launch of each kernel from event timers, the median of --repeats windows after a warm-up, every window, and the
library's launch record.  The tool fixes no number.

    python tools/pyin_timing.py [--batch 64] [--seconds 6.5] [--repeats 5] [--inner 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per kernel")
    ap.add_argument("--inner", type=int, default=5, help="launches per timed window")
    args = ap.parse_args()
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib, features as FX, pitch as PX

    assert torch.cuda.is_available(), "pyin_timing.py measures on a GPU: there is no fallback"
    dev = torch.device("cuda:0")
    pl = PX.PitchPlan(dev, method="pyin")
    rng = np.random.RandomState(7)
    mean = args.seconds * pl.fs
    lens = [int(n) for n in rng.randint(int(0.75 * mean), int(1.25 * mean) + 1, size=args.batch)]
    with torch.cuda.device(dev):
        g = torch.Generator(device=dev).manual_seed(7)
        phase = 2.0 * np.pi * 150.0 / pl.fs * torch.arange(sum(lens), device=dev, dtype=torch.float64)
        tone = sum(a * torch.sin((k + 1) * phase) for k, a in enumerate((1.0, 0.6, 0.4, 0.3, 0.2, 0.1)))
        packed = (0.2 * tone).float() + (torch.rand(sum(lens), device=dev, generator=g) - 0.5) * 0.2
    mp = FX.Maps(lens, pl.hop, dev)
    new = lambda *shape, **kw: torch.empty(*shape, device=dev, dtype=kw.get("dtype", torch.float32))
    yin, raw, cm = new(mp.frames), new(mp.frames), new(mp.frames, pl.n_lag)
    lv, lu, bf0 = new(mp.frames, pl.nb), new(mp.frames), new(mp.frames, pl.nb)
    state, score, ws = new(mp.frames, dtype=torch.int32), new(mp.n_utt), new(pl.workspace_bytes(mp.frames), dtype=torch.uint8)
    legs = {"px_yin_kernel<1024>": lambda: PX.launch_yin(pl, mp, packed, yin, cm),
            "pyin_obs_kernel": lambda: PX.launch_pyin_obs(pl, mp, cm, lv, lu, bf0),
            "pyin_viterbi_kernel": lambda: PX.launch_pyin_viterbi(pl, mp, lv, lu, bf0, ws, state, raw, score)}
    times = {k: [] for k in legs}
    for fn in legs.values():  # in order: each launch reads what the one before wrote
        for _ in range(2):
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
    print(json.dumps(dict(batch=args.batch, samples=sum(lens), frames=mp.frames, longest_utterance_frames=max(mp.lens), nb=pl.nb, band=pl.band,
                          voiced_frames=int((raw > 0).sum()), ms={k: [round(t, 4) for t in v] for k, v in times.items()},
                          median_ms={k: round(float(np.median(v)), 4) for k, v in times.items()},
                          launch_record_ms={k: round(v["ms"] / max(v["launches"], 1), 4) for k, v in rec.items() if k in legs})))


if __name__ == "__main__":
    main()
