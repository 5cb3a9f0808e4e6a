"""A/B of the two ways to run the Parallel WaveGAN discriminator on one MI355X: Parallel WaveGAN's training shape, batch 6 x 25 600
samples, the default architecture (10 layers, 64 channels, kernel size 3), random weights, no weight norm on either leg.

  A  the same stack built from torch.nn.Conv1d + LeakyReLU in float32 torch-ROCm eager on the [6, 1, 25600] batch
  B  ParallelWaveGANDiscriminator (the pwd_* kernels) on the same batch

Three cases per leg: the forward pass alone (no_grad); forward + backward with frozen weights (the generator's update: the waveform gradient only);
forward + backward with weight gradients and a detached input (the discriminator's update).  One process, alternating legs, event timers, a synchronise
at each end, medians.  Prints one JSON line.

    python tools/pwgd_ab.py [--batch 6] [--samples 25600] [--repeats 20] [--warmup 3] [--prof] [--dump PATH]

--dump PATH saves leg B's scores, waveform gradient and weight gradients of this fixed-seed run as PATH (.npy, one float32 vector): two builds of the
library computed the same bits where np.array_equal of their dumps holds.
"""
import argparse
import copy
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b), out


def eager_stack(layers=10, channels=64, k=3, slope=0.2):
    mods = []
    for i in range(layers - 1):
        d = max(i, 1)
        mods += [torch.nn.Conv1d(1 if i == 0 else channels, channels, k, dilation=d, padding=(k - 1) // 2 * d), torch.nn.LeakyReLU(slope)]
    return torch.nn.Sequential(*mods, torch.nn.Conv1d(channels, 1, k, padding=(k - 1) // 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=6)
    ap.add_argument("--samples", type=int, default=25600)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--prof", action="store_true", help="also one profiled discriminator update of leg B: per-kernel ms and TFLOP/s from the library's launch record")
    ap.add_argument("--dump", metavar="PATH", help="save leg B's scores and all gradients of the fixed-seed run as one .npy vector")
    args = ap.parse_args()
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib, pwg_discriminator as P

    dev = torch.device("cuda:0")
    torch.manual_seed(7)
    hip = P.ParallelWaveGANDiscriminator(use_weight_norm=False).to(dev)
    eager = eager_stack().to(dev)
    with torch.no_grad():  # the same weights on both legs
        for c, m in zip(hip.convs(), [m for m in eager if isinstance(m, torch.nn.Conv1d)]):
            c.bias.normal_(0, 0.1)
            m.weight.copy_(c.weight), m.bias.copy_(c.bias)
    x = torch.randn(args.batch, 1, args.samples, device=dev).clamp_(-1, 1)

    def forward(mod):
        with torch.no_grad():
            return mod(x)

    def frozen(mod):
        for p in mod.parameters():
            p.requires_grad_(False)
        xr = x.clone().requires_grad_(True)
        P.generator_adversarial_loss(mod(xr)).backward()
        return xr.grad

    def update(mod):
        for p in mod.parameters():
            p.requires_grad_(True)
            p.grad = None
        P.generator_adversarial_loss(mod(x)).backward()
        return [p.grad for p in mod.parameters()]

    cases = dict(forward=forward, backward_frozen_weights=frozen, backward_weight_gradients=update)
    legs = {"%s/%s" % (c, leg): (lambda fn=fn, mod=mod: fn(mod)) for c, fn in cases.items() for leg, mod in (("A_eager_f32", eager), ("B_hip", hip))}
    times = {k: [] for k in legs}
    for _ in range(args.warmup):
        for fn in legs.values():
            fn()
            torch.cuda.synchronize(dev)
    for _ in range(args.repeats):
        for k, fn in legs.items():  # alternating legs
            times[k].append(timed(fn, dev)[0])
    med = {k: round(float(np.median(v)), 3) for k, v in times.items()}
    out = dict(batch=args.batch, samples=args.samples, repeats=args.repeats, median_ms=med, min_ms={k: round(float(np.min(v)), 3) for k, v in times.items()},
               A_over_B={c: round(med[c + "/A_eager_f32"] / med[c + "/B_hip"], 3) for c in cases})
    # the two legs compute the same scores and gradients
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    ga, gb = frozen(hip), frozen(eager)
    out["max_rel_A_minus_B"] = dict(scores=rel(forward(hip), forward(eager)), waveform_gradient=rel(ga, gb),
                                    weight_gradients=max(rel(a, b) for a, b in zip(update(hip), update(eager))))
    # two float32 paths round a pre-activation next to zero to different sides in a few of the batch * samples * 576 cells, and each such cell flips a
    # LeakyReLU mask for the 77 samples under it: the waveform gradient's maximum shows these, its 2-norm and the share of samples hit do not
    out["waveform_gradient"] = dict(rel_2norm=float((ga - gb).norm() / gb.norm()), share_of_samples_off_by_1e_4_of_max=float(((ga - gb).abs() > 1e-4 * gb.abs().max()).float().mean()))
    ref = copy.deepcopy(eager).double()  # the same stack in float64: each float32 leg's distance from it
    x64 = x.double().requires_grad_(True)
    P.generator_adversarial_loss(ref(x64)).backward()
    out["waveform_gradient"]["rel_2norm_vs_float64"] = {k: float((g.double() - x64.grad).norm() / x64.grad.norm()) for k, g in (("A_eager_f32", gb), ("B_hip", ga))}
    if args.dump:
        np.save(args.dump, torch.cat([v.detach().reshape(-1) for v in [forward(hip), ga] + update(hip)]).cpu().numpy())
    if args.prof:
        _lib.prof_enable(True)
        update(hip)
        frozen(hip)
        torch.cuda.synchronize(dev)
        rec = _lib.prof_collect()
        _lib.prof_enable(False)
        out["kernels"] = {k: dict(launches=v["launches"], ms=round(v["ms"], 3), tflops=round(v["flops"] / max(v["ms"], 1e-9) / 1e9, 2)) for k, v in rec.items()
                          if k.startswith("pwd_")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
