"""A/B of the two ways to run a HiFi-GAN v1 checkpoint on one MI355X: 64 utterances, random weights (tests/hifigan_ref.py).

  A  the float32 torch-ROCm eager module of the same architecture (hifigan_ref.TorchHiFiGAN) on the zero-padded [64, 80, T_max] batch
  B  HiFiGANGenerator.synthesize_packed on the packed rows, in default (bf16x3) and FCL_GEMM_BF16 mode
  (for orientation) the Parallel WaveGAN generator on the same frames

One process, alternating legs, event timers, a synchronise at each batch end.  Prints one JSON line.

    python tools/hifigan_ab.py [--batch 64] [--frames-lo 420] [--frames-hi 720] [--repeats 5] [--prof]

--speech: the text -> waveform A/B of this generator instead, under the protocol of tools/speech_ab.py (whose remaining flags follow: --batch,
--batches, --repeats, --distinct, --t-lo, --t-hi, --alone): leg A BatchRunner -> frames() -> synthesize_packed -> float32 D2H, leg B SpeechRunner on
hifigan.CapacitySynth -> int16 D2H; wall ms per batch, RTF, host-enqueue ms per batch, and the generator alone in both forms (exact vs capacity)
from the library's event timers, `blocks_ms` = the residual-unit kernels.

    python tools/hifigan_ab.py --speech [--batch 64] [--batches 20] [--repeats 3]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))


def timed(fn, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b), out


def speech(argv):
    """the SpeechRunner leg: tools/speech_ab.py with a HiFi-GAN v1 generator (random weights, as the legs above)"""
    import hifigan_ref as R
    import speech_ab
    from fcl_taco2_amd import hifigan

    make = lambda dev: hifigan.HiFiGANGenerator(hifigan.HiFiGANPlan(R.random_state_dict(np.random.RandomState(7), R.V1), dev, R.plan_cfg(R.V1)))
    speech_ab.main(argv, make_gen=make, blocks_prefix="hfg_unit")


def main():
    if "--speech" in sys.argv[1:]:
        return speech([a for a in sys.argv[1:] if a != "--speech"])
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames-lo", type=int, default=420)
    ap.add_argument("--frames-hi", type=int, default=720)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-eager", action="store_true", help="leg B only (a kernel-trace run)")
    ap.add_argument("--prof", action="store_true", help="also one profiled pass of leg B: per-kernel ms and TFLOP/s from the library's launch record")
    args = ap.parse_args()
    import fcl_taco2_amd  # noqa: F401
    import hifigan_ref as R
    from fcl_taco2_amd import _lib, hifigan, ops, vocoder

    dev = torch.device("cuda:0")
    rng = np.random.RandomState(7)
    lens = [int(n) for n in rng.randint(args.frames_lo, args.frames_hi + 1, size=args.batch)]
    sd = R.random_state_dict(rng, R.V1)
    mels = [rng.standard_normal((n, 80)).astype(np.float32) for n in lens]
    rows = torch.from_numpy(np.concatenate(mels)).to(dev)
    gen = hifigan.HiFiGANGenerator(hifigan.HiFiGANPlan(sd, dev, R.plan_cfg(R.V1)))
    hop, frames = gen.plan.hop, sum(lens)
    legs = {}
    if not args.skip_eager:
        mod = R.TorchHiFiGAN(sd, R.V1).to(dev)
        padded = torch.zeros(args.batch, 80, max(lens), device=dev)
        for i, m in enumerate(mels):
            padded[i, :, : lens[i]] = torch.from_numpy(m.T).to(dev)
        with torch.no_grad():
            legs["A_eager_f32_padded"] = lambda: mod(padded)
    legs["B_default"] = lambda: gen.synthesize_packed(rows, lens)

    def b_bf16():
        with ops.gemm_mode("bf16"):
            return gen.synthesize_packed(rows, lens)

    legs["B_bf16"] = b_bf16
    if not args.skip_eager:
        import helpers as H

        pwg = vocoder.ParallelWaveGANGenerator(vocoder.PWGPlan(H.pwg_random_state_dict(np.random.RandomState(1), None, 1.0), dev))
        legs["PWG_same_frames"] = lambda: pwg.synthesize_packed(rows, lens, seed=1)
    times = {k: [] for k in legs}
    with torch.no_grad():
        for k, fn in legs.items():  # warm-up: one-time setup, allocator, solver choice of the eager module
            fn()
            torch.cuda.synchronize(dev)
        for _ in range(args.repeats):
            for k, fn in legs.items():  # alternating legs
                times[k].append(timed(fn, dev)[0])
    out = dict(batch=args.batch, frames=frames, samples=frames * hop, padded_samples=max(lens) * hop * args.batch, audio_s=frames * hop / 22050.0,
               ms={k: [round(t, 2) for t in v] for k, v in times.items()}, median_ms={k: round(float(np.median(v)), 2) for k, v in times.items()})
    out["rtf"] = {k: round(v / 1000.0 / out["audio_s"], 6) for k, v in out["median_ms"].items()}
    if not args.skip_eager:  # the two legs compute the same waveform
        with torch.no_grad():
            wa = legs["A_eager_f32_padded"]()
        wb = gen.synthesize_packed(rows, lens)
        # (the padded batch lets the bias-driven activations behind an utterance's end leak into its last frames -- the generator's receptive field is
        # ~15 frames -- so the legs are compared up to 24 frames before each end, and on the whole of the longest utterance, which has no padding)
        out["max_abs_A_minus_B"] = max(float((wa[i, 0, : (lens[i] - 24) * hop] - wb[i][: (lens[i] - 24) * hop]).abs().max()) for i in range(0, args.batch, 8))
        i = int(np.argmax(lens))
        out["max_abs_A_minus_B_longest"] = float((wa[i, 0, : lens[i] * hop] - wb[i]).abs().max())
    if args.prof:
        _lib.prof_enable(True)
        gen.synthesize_packed(rows, lens)
        torch.cuda.synchronize(dev)
        rec = _lib.prof_collect()
        _lib.prof_enable(False)
        out["kernels"] = {k: dict(launches=v["launches"], ms=round(v["ms"], 3), tflops=round(v["flops"] / max(v["ms"], 1e-9) / 1e9, 1)) for k, v in rec.items()
                          if k.startswith("hfg_")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
