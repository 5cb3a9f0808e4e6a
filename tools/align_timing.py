"""Timing of one forced-alignment E-step on one MI355X: `--utts` utterances of about `--frames` frames and `--phonemes` phonemes of
3 states, an inventory of 70 phonemes (M = 210), D = 28, features drawn around a random model along a random segmentation.

  A  the float64 numpy statement of tests/align_ref.py on the host: log-likelihoods, the recurrence one frame at a time, backtrack (timed on
     `--ref-utts` utterances and scaled)
  B  the three launches of csrc/align.hip on maps and buffers prepared ahead of time: al_loglik_kernel, al_viterbi_kernel, al_stats_kernel
  largest  the largest utterance the kernel takes, S = 1024 rows x T = 4096 frames, M = 1024: the Viterbi launch alone
  lattice  the same chains of B (and the largest utterance) written as lattices through al_lattice_viterbi_kernel of
     csrc/align_lattice.hip: `lattice_viterbi_ms`, its ratio to `viterbi_ms`, and whether both entries gave the same alignment
  C  with `--mixtures C [C ...]`: the same E-step with C components in every state, the three launches of csrc/align_gmm.hip --
     al_gmm_loglik_kernel, al_gmm_post_kernel, al_gmm_stats_kernel -- around the same Viterbi launch, on the alignment B gave

One process, event timers, a warm-up launch of every shape, the median of `--repeats`.  Prints one JSON line.  The tool fixes no number.

    python tools/align_timing.py [--utts 64] [--frames 800] [--phonemes 40] [--repeats 5] [--ref-utts 2] [--mixtures 4 8]
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


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--frames", type=int, default=800, help="mean length; lengths are drawn within +- 25 %% of it")
    ap.add_argument("--phonemes", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ref-utts", type=int, default=2, help="utterances the float64 statement is timed on")
    ap.add_argument("--mixtures", type=int, nargs="*", default=[], metavar="C", help="also time the mixture E-step with C components per state, 1 .. 8")
    args = ap.parse_args()
    assert all(1 <= c <= 8 for c in args.mixtures), "--mixtures takes component counts in 1 .. 8"
    import align_ref as R
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import alignment as A

    assert torch.cuda.is_available(), "align_timing.py measures on a GPU: there is no fallback"
    dev, K, P, D = "cuda:0", 3, 70, 28
    M = P * K
    rng = np.random.RandomState(0)
    mean, var = rng.randn(M, D) * 2.0, rng.uniform(0.5, 2.0, (M, D))
    feats, graphs = [], []
    for _ in range(args.utts):
        T = int(args.frames * rng.uniform(0.75, 1.25))
        row_state, row_skip, _ = R.graph(list(rng.randint(0, P, args.phonemes)), [False] * args.phonemes, K)
        counts = R.uniform_alignment(T, row_skip)
        feats.append((mean[np.repeat(row_state, counts)] + rng.randn(T, D) * np.sqrt(var[np.repeat(row_state, counts)])).astype(np.float32))
        graphs.append((row_state, row_skip))
    mp = A.AlignMaps([len(x) for x in feats], graphs, M, dev)
    params = tuple(torch.from_numpy(a).to(dev) for a in R.params32(mean, var))
    x = torch.from_numpy(np.concatenate(feats)).to(dev)
    ll = torch.empty(mp.frames, M, device=dev)
    ws = torch.empty(mp.workspace_bytes(), device=dev, dtype=torch.uint8)
    i32 = lambda n: torch.empty(n, device=dev, dtype=torch.int32)
    frame_row, row_begin, row_frames, ok, score = i32(mp.frames), i32(mp.rows), i32(mp.rows), i32(mp.n_utt), torch.empty(mp.n_utt, device=dev)
    acc = (torch.zeros(M, device=dev, dtype=torch.int64), torch.zeros(M, D, device=dev, dtype=torch.float64), torch.zeros(M, D, device=dev, dtype=torch.float64))
    out = dict(utts=args.utts, frames=mp.frames, rows=mp.rows, cells=mp.cells, states=M, dim=D)
    out["loglik_ms"] = timed(lambda: A.launch_loglik(params, x, ll, mp.frames), args.repeats)
    out["viterbi_ms"] = timed(lambda: A.launch_viterbi(mp, ll, ws, frame_row, row_begin, row_frames, score, ok), args.repeats)
    out["stats_ms"] = timed(lambda: A.launch_stats(mp, x, row_begin, row_frames, *acc), args.repeats)
    assert bool(ok.cpu().numpy().all())
    import align_lattice_ref as LR

    lmp = A.AlignMaps([len(x) for x in feats], [(rs,) + LR.chain_as_lattice(sk) for rs, sk in graphs], M, dev)
    l_frame_row, l_row_begin, l_row_frames, l_ok, l_score = i32(mp.frames), i32(mp.rows), i32(mp.rows), i32(mp.n_utt), torch.empty(mp.n_utt, device=dev)
    out["lattice_viterbi_ms"] = timed(lambda: A.launch_lattice_viterbi(lmp, ll, ws, l_frame_row, l_row_begin, l_row_frames, l_score, l_ok), args.repeats)
    out["lattice_over_chain"] = out["lattice_viterbi_ms"] / out["viterbi_ms"]
    out["lattice_same_as_chain"] = bool(torch.equal(l_frame_row, frame_row) and torch.equal(l_row_frames, row_frames) and torch.equal(l_score, score))
    t0 = time.perf_counter()
    same = True
    for k in range(args.ref_utts):
        r = R.viterbi(R.loglik(feats[k], *R.params32(mean, var))[0], *graphs[k])
        same = same and np.array_equal(r["row_frames"], row_frames.cpu().numpy()[mp.row_offs[k] : mp.row_offs[k + 1]])
    out["float64_ms_scaled"] = (time.perf_counter() - t0) * 1e3 * args.utts / args.ref_utts
    out["same_alignment_as_float64"] = bool(same)
    # the mixture E-step: C components per state around the state's mean, equal weights, on the alignment the launches above left
    fs = A.frame_states(mp, frame_row)
    for c in args.mixtures:
        comp_off = np.arange(M + 1, dtype=np.int32) * c
        gm = A.AlignModel(["p%d" % i for i in range(P)], K, np.repeat(mean, c, axis=0) + rng.randn(M * c, D) * 0.5, np.repeat(var, c, axis=0),
                          weight=np.full(M * c, 1.0 / c), comp_off=comp_off)
        gp = tuple(torch.from_numpy(a).to(dev) for a in gm.gmm_params32())
        gamma = torch.empty(mp.frames, 8, device=dev)
        gacc = (torch.zeros(M * c, device=dev, dtype=torch.float64), torch.zeros(M * c, D, device=dev, dtype=torch.float64),
                torch.zeros(M * c, D, device=dev, dtype=torch.float64))
        out["mixtures_%d" % c] = dict(
            components=M * c,
            loglik_ms=timed(lambda: A.launch_gmm_loglik(gp, x, ll, mp.frames, c), args.repeats),
            post_ms=timed(lambda: A.launch_gmm_post(gp, x, fs, gamma, mp.frames, c), args.repeats),
            stats_ms=timed(lambda: A.launch_gmm_stats(mp, gp[3], x, gamma, row_begin, row_frames, *gacc, max_comp=c), args.repeats))
    # the largest utterance
    S, T = 1024, 4096
    big = A.AlignMaps([T], [(np.arange(S, dtype=np.int32), np.zeros(S, np.int32))], S, dev)
    llb = torch.randn(T, S, device=dev) * 2.0 - 30.0
    wsb = torch.empty(big.workspace_bytes(), device=dev, dtype=torch.uint8)
    fb, rb, rf, okb, sb = i32(T), i32(S), i32(S), i32(1), torch.empty(1, device=dev)
    out["largest_viterbi_ms"] = timed(lambda: A.launch_viterbi(big, llb, wsb, fb, rb, rf, sb, okb), args.repeats)
    lbig = A.AlignMaps([T], [(np.arange(S, dtype=np.int32),) + LR.chain_as_lattice(np.zeros(S, np.int32))], S, dev)
    out["largest_lattice_viterbi_ms"] = timed(lambda: A.launch_lattice_viterbi(lbig, llb, wsb, fb, rb, rf, sb, okb), args.repeats)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
