"""A/B of the two ways to train the Parallel WaveGAN generator on one MI355X: Parallel WaveGAN's training shape, batch 6 x 25 600
samples (100 frames at hop 256 + 2 x 2 of context), the v1 geometry (30 blocks in 3 stacks, 64 residual / skip channels, 80 aux channels, kernel size 3),
the same random weights on both legs, no weight norm on either.

  A  oracle.pwg_oracle.generator_forward (F.conv1d per layer) under torch autograd in float32 on the device
  B  TrainableParallelWaveGANGenerator (the pwt_* kernels under the residual stack, torch operations around it)

Three cases per leg: the forward pass alone (no_grad); forward + backward (every parameter's gradient); forward + backward + one Adam step.  One
process, alternating legs, event timers, a synchronise at each end, medians.  Prints one JSON line.

    python tools/pwgg_ab.py [--batch 6] [--frames 100] [--repeats 20] [--warmup 3] [--prof] [--dump PATH] [--ends]

--ends times two other legs by the same protocol, two copies of leg B's module that differ in the generator's ends alone:

  T  forward(z, c, ends="torch"): the upsampling network, first_conv and the last layers as torch operations (the path before the pwe_* kernels)
  H  forward(z, c, ends="hip"):   the same in the pwe_* kernels of csrc/pwg_ends.hip

and adds `outside_ms`, a by-operation account of the host-side work around the kernels at this geometry (medians of the same number of rounds): the
weight-norm folds of a weight-norm module, pack_weights, and unpack_dweights.

--dump PATH saves leg B's waveform and every parameter's gradient of this fixed-seed run (before any Adam step) as PATH (.npy, one float32 vector): two
builds of the library computed the same bits where np.array_equal of their dumps holds -- apart from the gradients of first_conv and the upsampling
network, torch's own convolution weight gradients, which differ in the last bits between two runs of one build.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CEILING_TFLOPS = 157.0  # exact-fp32 MFMA rate of the MI355X


def timed(fn, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=6)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--prof", action="store_true", help="also one profiled forward + backward of leg B: per-kernel ms and TFLOP/s from the library's launch record")
    ap.add_argument("--ends", action="store_true", help="time the module with torch ends against the module with HIP ends (legs T and H) instead of A and B")
    ap.add_argument("--dump", metavar="PATH", help="save leg B's waveform and all gradients of the fixed-seed run as one .npy vector")
    args = ap.parse_args()
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib, pwg_generator as G
    from oracle import pwg_oracle as O

    dev = torch.device("cuda:0")
    torch.manual_seed(7)
    hip = G.TrainableParallelWaveGANGenerator(use_weight_norm=False).to(dev)
    with torch.no_grad():
        for k, p in hip.named_parameters():
            if k.endswith("bias"):
                p.normal_(0, 0.1)
    eager = {k: v.detach().clone().requires_grad_(True) for k, v in hip.state_dict().items()}  # the same weights on both legs
    T = args.frames * hip.hop
    z = torch.randn(args.batch, 1, T, device=dev)
    c = torch.randn(args.batch, 80, args.frames + 2 * hip.ctx, device=dev)
    opt = {"A_eager_f32": torch.optim.Adam(list(eager.values()), 1e-4), "B_hip": torch.optim.Adam(hip.parameters(), 1e-4)}
    run = {"A_eager_f32": lambda: O.generator_forward(eager, z, O.upsample(eager, c)), "B_hip": lambda: hip(z, c)}
    params = {"A_eager_f32": list(eager.values()), "B_hip": list(hip.parameters())}
    first, second = "A_eager_f32", "B_hip"
    if args.ends:
        import copy

        other = copy.deepcopy(hip)
        first, second = "T_torch_ends", "H_hip_ends"
        opt = {first: torch.optim.Adam(other.parameters(), 1e-4), second: opt["B_hip"]}
        run = {first: lambda: other(z, c, ends="torch"), second: lambda: hip(z, c, ends="hip")}
        params = {first: list(other.parameters()), second: list(hip.parameters())}

    def forward(leg):
        with torch.no_grad():
            return run[leg]()

    def backward(leg):
        for p in params[leg]:
            p.grad = None
        run[leg]().square().mean().backward()
        return [p.grad for p in params[leg]]

    def step(leg):
        backward(leg)
        opt[leg].step()

    cases = dict(forward=forward, forward_backward=backward, forward_backward_adam=step)
    legs = {"%s/%s" % (c_, leg): (lambda fn=fn, leg=leg: fn(leg)) for c_, fn in cases.items() for leg in run}
    # the two legs compute the same waveform and gradients (before any Adam step moves them apart)
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    out = dict(batch=args.batch, samples=T, repeats=args.repeats)
    ga, gb = backward(first), backward(second)
    dead = [i for i, (k, _) in enumerate(hip.named_parameters()) if k.startswith("conv_layers.%d.conv1x1_out" % (hip.config["layers"] - 1))]
    out["max_rel_H_minus_T" if args.ends else "max_rel_B_minus_A"] = dict(waveform=rel(forward(second), forward(first)),
                                    gradients=max(rel(b, a) for i, (a, b) in enumerate(zip(ga, gb)) if i not in dead),
                                    last_block_out_gradient_zero=all(not gb[i].any() and (ga[i] is None or not ga[i].any()) for i in dead))
    if args.dump:
        np.save(args.dump, torch.cat([v.detach().reshape(-1) for v in [forward(second)] + gb]).cpu().numpy())
    times = {k: [] for k in legs}
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
            torch.cuda.synchronize(dev)
    for _ in range(args.repeats):
        for k, fn in legs.items():  # alternating legs
            times[k].append(timed(fn, dev)[0])
    med = {k: round(float(np.median(v)), 3) for k, v in times.items()}
    out.update(median_ms=med, min_ms={k: round(float(np.min(v)), 3) for k, v in times.items()},
               spread_ms={k: round(float(np.percentile(v, 75) - np.percentile(v, 25)), 3) for k, v in times.items()},
               **{"T_over_H" if args.ends else "A_over_B": {c_: round(med[c_ + "/" + first] / med[c_ + "/" + second], 3) for c_ in cases}})
    if args.prof:
        _lib.prof_enable(True)
        backward(second)
        torch.cuda.synchronize(dev)
        rec = _lib.prof_collect()
        _lib.prof_enable(False)
        out["kernels"] = {k: dict(launches=v["launches"], ms=round(v["ms"], 3), tflops=round(v["flops"] / max(v["ms"], 1e-9) / 1e9, 2),
                                  of_ceiling=round(v["flops"] / max(v["ms"], 1e-9) / 1e9 / CEILING_TFLOPS, 3)) for k, v in rec.items() if k.startswith(("pwt_", "pwe_"))}
        out["kept_bytes"] = hip.plan().kept_bytes(args.batch * T)
    if args.ends:
        wn = G.TrainableParallelWaveGANGenerator(use_weight_norm=True).to(dev)
        plan, plain = hip.plan(), [blk.plain() for blk in hip.conv_layers]
        dws = [tuple(torch.empty(s_, device=dev) for s_ in plan.dweight_shapes()) for _ in plain]
        ops_ = dict(weight_norm_folds=lambda: [m.folded() for _, m in wn.convs()], pack_weights=lambda: G.pack_weights(plain),
                    unpack_dweights=lambda: [G.unpack_dweights(plan, *d) for d in dws])
        acc = {k: [] for k in ops_}
        for r in range(args.warmup + args.repeats):
            for k, fn in ops_.items():
                ms = timed(fn, dev)[0]
                if r >= args.warmup:
                    acc[k].append(ms)
        out["outside_ms"] = {k: round(float(np.median(v)), 3) for k, v in acc.items()}
        out["outside_ms"]["folded_convolutions"] = len(wn.convs())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
