"""A/B of the two ways to run the HiFi-GAN multi-period discriminator on one MI355X: the published training shape, batch 16 x 8 192
samples, periods (2, 3, 5, 7, 11), the default widths (32 .. 1024), random weights, no weight norm on either leg.

  A  the same stacks built from torch.nn.Conv2d + LeakyReLU in float32 torch-ROCm eager on the reflection-padded [16, 1, H, p] views
  B  HiFiGANMultiPeriodDiscriminator (the hpd_* kernels) on the same batch

Three cases per leg: the forward pass alone (no_grad); forward + backward with frozen weights and feature-map gradients (the generator's update:
adversarial + 2 x feature matching against a fixed real batch's maps); forward + backward with weight gradients on a detached input (the
discriminator's update).  One process, alternating legs, event timers, a synchronise at each end, medians with the interquartile spread.  Prints one
JSON line and writes it to profiles/hfgd_ab.json.

    python tools/hfgd_ab.py [--batch 16] [--samples 8192] [--repeats 20] [--warmup 3] [--prof] [--dump PATH]

--dump PATH saves leg B's scores, waveform gradient and weight and bias gradients of this fixed-seed run as PATH (.npy, one float32 vector): two builds of
the library computed the same bits where np.array_equal of their dumps holds.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b), out


class EagerPeriod(torch.nn.Module):
    """one period discriminator as torch.nn.Conv2d + LeakyReLU; returns the maps in the package's [B, C, H, p] layout and the flattened scores"""

    def __init__(self, period, geometry, slope):
        super().__init__()
        self.period, self.slope = period, slope
        self.convs = torch.nn.ModuleList(torch.nn.Conv2d(ci, co, (k, 1), (s, 1), (pad, 0)) for ci, co, k, s, pad in geometry)

    def forward(self, x):
        B, _, T = x.shape
        if T % self.period:
            x = F.pad(x, (0, self.period - T % self.period), "reflect")
        h, outs = x.view(B, 1, -1, self.period), []
        for i, conv in enumerate(self.convs):
            h = conv(h)
            if i < len(self.convs) - 1:
                h = F.leaky_relu(h, self.slope)
                outs.append(h)
        return outs + [torch.flatten(h, 1, -1)]


class EagerMPD(torch.nn.Module):
    def __init__(self, hip, P):
        super().__init__()
        self.discriminators = torch.nn.ModuleList(EagerPeriod(d.period, P.check_configuration(**d.config), d.config["negative_slope"])
                                                  for d in hip.discriminators)

    def forward(self, x):
        return [d(x) for d in self.discriminators]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--samples", type=int, default=8192)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--prof", action="store_true", help="also one profiled update of each kind of leg B: per-kernel ms and TFLOP/s from the library's launch record")
    ap.add_argument("--dump", metavar="PATH", help="save leg B's scores and all gradients of the fixed-seed run as one .npy vector")
    args = ap.parse_args()
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib, hifigan_discriminator as P

    dev = torch.device("cuda:0")
    torch.manual_seed(7)
    hip = P.HiFiGANMultiPeriodDiscriminator(discriminator_params=dict(use_weight_norm=False)).to(dev)
    eager = EagerMPD(hip, P).to(dev)
    with torch.no_grad():  # the same weights on both legs
        for dh, de in zip(hip.discriminators, eager.discriminators):
            for c, m in zip(dh.conv_list(), de.convs):
                c.bias.normal_(0, 0.1)
                m.weight.copy_(c.weight), m.bias.copy_(c.bias)
    x = torch.randn(args.batch, 1, args.samples, device=dev).clamp_(-1, 1)
    y = torch.randn(args.batch, 1, args.samples, device=dev).clamp_(-1, 1)
    with torch.no_grad():
        real = {id(hip): hip(y), id(eager): eager(y)}

    def forward(mod):
        with torch.no_grad():
            return mod(x)

    def frozen(mod):
        for p in mod.parameters():
            p.requires_grad_(False)
        xr = x.clone().requires_grad_(True)
        outs = mod(xr)
        (P.generator_adversarial_loss(outs) + 2.0 * P.feature_match_loss(outs, real[id(mod)])).backward()
        return xr.grad

    def update(mod):
        for p in mod.parameters():
            p.requires_grad_(True)
            p.grad = None
        r, f = P.discriminator_adversarial_loss(mod(y), mod(x))
        (r + f).backward()
        return [p.grad for p in mod.parameters()]

    cases = dict(forward=forward, backward_frozen_weights_feature_maps=frozen, backward_weight_gradients=update)
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
    iqr = {k: round(float(np.percentile(v, 75) - np.percentile(v, 25)), 3) for k, v in times.items()}
    out = dict(batch=args.batch, samples=args.samples, repeats=args.repeats, median_ms=med, iqr_ms=iqr,
               A_over_B={c: round(med[c + "/A_eager_f32"] / med[c + "/B_hip"], 3) for c in cases})
    # the two legs compute the same scores, maps and gradients (leg B's outputs are packed: compared through the package's views)
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    oh, oe = forward(hip), forward(eager)
    views = [P.to_reference_layout(o, d.period, args.batch) for o, d in zip(oh, hip.discriminators)]
    ga, gb = frozen(hip), frozen(eager)
    out["max_rel_A_minus_B"] = dict(maps_and_scores=max(rel(a, b) for va, vb in zip(views, oe) for a, b in zip(va, vb)),
                                    weight_gradients=max(rel(a, b) for a, b in zip(update(hip), update(eager))))
    # a LeakyReLU mask or an L1 sign next to zero can fall to different sides on two float32 paths: the gradient's 2-norm, not its maximum, is compared
    out["waveform_gradient_rel_2norm_A_minus_B"] = float((ga - gb).norm() / gb.norm())
    if args.dump:
        np.save(args.dump, torch.cat([v.detach().reshape(-1) for v in [o[-1] for o in oh] + [ga] + update(hip)]).cpu().numpy())
    if args.prof:
        _lib.prof_enable(True)
        update(hip)
        frozen(hip)
        torch.cuda.synchronize(dev)
        rec = _lib.prof_collect()
        _lib.prof_enable(False)
        out["kernels"] = {k: dict(launches=v["launches"], ms=round(v["ms"], 3), tflops=round(v["flops"] / max(v["ms"], 1e-9) / 1e9, 2)) for k, v in rec.items()
                          if k.startswith("hpd_")}
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "hfgd_ab.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
