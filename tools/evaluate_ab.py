"""A/B of one evaluation batch on one MI355X: `--pairs` pairs of mel sequences of about `--frames` frames (a random walk in the
log-mel domain against a jittered, repeated-frame warp of it plus noise), order 13.

  A  the float64 numpy statement of tests/evaluate_ref.py on the host: cepstra, distances, the recurrence one anti-diagonal at a time, backtrack
     (timed on `--ref-pairs` pairs and scaled: it takes seconds)
  B  Evaluator.compare_mels on the device: two cepstra launches, one DTW launch, host copies of the figures -- the call a driver makes
  B_launch_only  the DTW launch alone on maps and buffers prepared ahead of time

One process, event timers for B, a synchronise at each batch end.  Prints one JSON line: ms per batch of each leg, the kernels' ms from the library's
launch record, and the largest difference of the two legs' MCD.  The tool fixes no number.

    python tools/evaluate_ab.py [--pairs 64] [--frames 800] [--repeats 5] [--ref-pairs 4]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--frames", type=int, default=800, help="mean length; lengths are drawn within +- 25 %% of it")
    ap.add_argument("--order", type=int, default=13)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ref-pairs", type=int, default=4, help="pairs the float64 statement is timed on")
    args = ap.parse_args()
    import evaluate_ref as E
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib, metrics as M

    assert torch.cuda.is_available(), "evaluate_ab.py measures on a GPU: there is no fallback"
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(3)
    N = 80
    la = [int(n) for n in rng.randint(int(0.75 * args.frames), int(1.25 * args.frames) + 1, size=args.pairs)]
    lb = [int(n) for n in rng.randint(int(0.75 * args.frames), int(1.25 * args.frames) + 1, size=args.pairs)]
    xa, xb = [], []
    for ta, tb in zip(la, lb):
        a = (-3.0 + np.cumsum(0.1 * rng.randn(ta, N), axis=0) + 0.5 * rng.randn(1, N)).astype(np.float32)
        idx = np.sort(np.clip(np.rint(np.linspace(0, ta - 1, tb) + rng.uniform(-1.5, 1.5, tb)), 0, ta - 1).astype(np.int64))
        xa.append(a)
        xb.append((a[idx] + 0.05 * rng.randn(tb, N)).astype(np.float32))
    ev = M.Evaluator(dev, N, args.order)
    ra, rb = torch.from_numpy(np.concatenate(xa)).to(dev), torch.from_numpy(np.concatenate(xb)).to(dev)
    leg_b = lambda: ev.compare_mels(ra, la, rb, lb)
    mp = M.PairMaps(la, lb, dev)
    ca, cb = ev.cepstra(ev.raw_plan, ra), ev.cepstra(ev.raw_plan, rb)
    ws = torch.empty(mp.workspace_bytes(), device=dev, dtype=torch.uint8)
    path, n, cost = torch.empty(mp.path_rows, 2, device=dev, dtype=torch.int32), torch.empty(mp.n_pairs, device=dev, dtype=torch.int32), torch.empty(mp.n_pairs, device=dev)
    leg_l = lambda: M.launch_dtw(mp, args.order, ca, cb, ws, path, n, cost)
    times = dict(B_hip=[], B_launch_only=[])
    for fn in (leg_b, leg_l):
        fn()
    torch.cuda.synchronize(dev)
    for _ in range(args.repeats):
        for k, fn in (("B_hip", leg_b), ("B_launch_only", leg_l)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            res = fn()
            e1.record()
            torch.cuda.synchronize(dev)
            times[k].append(e0.elapsed_time(e1))
            if k == "B_hip":
                got = res
    _lib.prof_enable(True)
    leg_b()
    torch.cuda.synchronize(dev)
    rec = _lib.prof_collect()
    _lib.prof_enable(False)
    table, bias = E.table_bias(N, args.order)
    t0 = time.perf_counter()
    want = []
    for k in range(min(args.ref_pairs, args.pairs)):
        c, p = E.dtw(E.cepstra(xa[k], table, bias)[0], E.cepstra(xb[k], table, bias)[0])
        want.append(E.mcd_db(c, len(p)))
    t_ref = (time.perf_counter() - t0) * 1e3
    cells_ref = sum(a * b for a, b in zip(la[: len(want)], lb[: len(want)]))
    out = dict(pairs=args.pairs, frames_a=sum(la), frames_b=sum(lb), cells=mp.cells, order=args.order,
               ms={k: [round(t, 3) for t in v] for k, v in times.items()}, median_ms={k: round(float(np.median(v)), 3) for k, v in times.items()},
               A_float64_numpy_ms_measured=round(t_ref, 1), A_pairs_measured=len(want), A_float64_numpy_ms_scaled_to_batch=round(t_ref * mp.cells / cells_ref, 1),
               kernels={k: dict(launches=v["launches"], ms=round(v["ms"], 4)) for k, v in rec.items() if k.startswith("ev_")},
               mcd_db_mean=float(np.mean(got["mcd_db"])), max_abs_mcd_diff_db=float(np.abs(np.asarray(want) - got["mcd_db"][: len(want)]).max()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
