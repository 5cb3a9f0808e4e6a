"""A/B of the two ways to run the HiFi-GAN generator in training on one MI355X: the v1 geometry on a batch of 16 x 8 192 samples
(32 frames at hop 256), the same random weights on both legs, no weight norm on either.

  A  tests/hifigan_ref.TorchHiFiGAN's expressions (F.conv1d / F.conv_transpose1d per layer) under torch autograd in float32 on the device, the
     parameters as leaves
  B  TrainableHiFiGANGenerator (input_conv and the stages in the hft_* kernels, the output end in torch)
  C  with --output-end: the same module with forward(output_end="hip"), the output end in the hfe_* kernels too

Two cases per leg: the forward pass alone (no_grad); forward + backward (every parameter's gradient).  One process, 3 warm-up rounds, 20 alternating
rounds between device events, a synchronise at each end, medians and the interquartile spread.  One profiled forward + backward of leg B gives the
per-kernel split from the library's launch record; `outside_kernels_ms` is leg B's forward + backward median less the kernels' sum (with
--output-end the same two figures for leg C under `hip_end`).  Prints one JSON line; --out PATH writes it there too.

    python tools/hfgg_ab.py [--batch 16] [--frames 32] [--repeats 20] [--warmup 3] [--output-end] [--out profiles/hfgg_ab.json]
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
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--output-end", action="store_true", help="add leg C: the module with its output end in HIP")
    ap.add_argument("--out", metavar="PATH")
    args = ap.parse_args()
    import fcl_taco2_amd  # noqa: F401
    import hifigan_ref as H
    from fcl_taco2_amd import _lib, hifigan_generator as G

    dev = torch.device("cuda:0")
    torch.manual_seed(7)
    sd = H.random_state_dict(np.random.RandomState(7), H.V1)
    hip = G.TrainableHiFiGANGenerator(use_weight_norm=False).to(dev)
    hip.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})

    class Eager(H.TorchHiFiGAN):  # the same expressions, the parameters as leaves
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.cfg = H.V1
            self.leaves = {k: torch.from_numpy(v).to(dev).requires_grad_(True) for k, v in sd.items()}

        def p(self, k):
            return self.leaves[k]

    eager = Eager()
    mel = torch.randn(args.batch, 80, args.frames, device=dev)
    run = {"A_eager_f32": lambda: eager(mel), "B_hip": lambda: hip(mel)}
    params = {"A_eager_f32": [eager.leaves[k] for k, _ in hip.named_parameters()], "B_hip": list(hip.parameters())}
    if args.output_end:
        run["C_hip_end"], params["C_hip_end"] = (lambda: hip(mel, output_end="hip")), params["B_hip"]

    def forward(leg):
        with torch.no_grad():
            return run[leg]()

    def backward(leg):
        for p in params[leg]:
            p.grad = None
        run[leg]().square().mean().backward()
        return [p.grad for p in params[leg]]

    cases = dict(forward=forward, forward_backward=backward)
    legs = {"%s/%s" % (c_, leg): (lambda fn=fn, leg=leg: fn(leg)) for c_, fn in cases.items() for leg in run}
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    out = dict(batch=args.batch, samples=args.frames * hip.hop, repeats=args.repeats, warmup=args.warmup)
    ga, gb = backward("A_eager_f32"), backward("B_hip")
    out["max_rel_B_minus_A"] = dict(waveform=rel(forward("B_hip"), forward("A_eager_f32")), gradients=max(rel(b, a) for a, b in zip(ga, gb)))
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
               A_over_B={c_: round(med[c_ + "/A_eager_f32"] / med[c_ + "/B_hip"], 3) for c_ in cases})

    def split(leg):
        """one profiled forward + backward -> (the launch record's hft_* / hfe_* entries, their sum, the leg's median less that sum)"""
        _lib.prof_enable(True)
        backward(leg)
        torch.cuda.synchronize(dev)
        rec = _lib.prof_collect()
        _lib.prof_enable(False)
        kernels = {k: dict(launches=v["launches"], ms=round(v["ms"], 3), tflops=round(v["flops"] / max(v["ms"], 1e-9) / 1e9, 2),
                           of_ceiling=round(v["flops"] / max(v["ms"], 1e-9) / 1e9 / CEILING_TFLOPS, 3)) for k, v in rec.items() if k.startswith(("hft_", "hfe_"))}
        total = round(sum(v["ms"] for v in kernels.values()), 3)
        return kernels, total, round(med["forward_backward/" + leg] - total, 3)

    out["kernels"], out["kernels_ms"], out["outside_kernels_ms"] = split("B_hip")
    if args.output_end:
        gc = backward("C_hip_end")
        k, total, outside = split("C_hip_end")
        out["hip_end"] = dict(kernels={n: v for n, v in k.items() if n.startswith("hfe_")}, kernels_ms=total, outside_kernels_ms=outside,
                              C_over_B={c_: round(med[c_ + "/C_hip_end"] / med[c_ + "/B_hip"], 3) for c_ in cases},
                              max_rel_C_minus_B=dict(waveform=rel(forward("C_hip_end"), forward("B_hip")), gradients=max(rel(c, b) for b, c in zip(gb, gc))))
    out["kept_bytes"] = hip.plan().kept_bytes(hip.maps([args.frames] * args.batch))
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
