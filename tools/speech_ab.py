"""A/B of the two in-process routes text -> waveform on one MI355X, BASELINE configs[4] shape: 64 utterances of 60 - 100 phonemes,
PREDICTED durations, FCL-taco2-S + Parallel WaveGAN v1, closed-form weights.

  A  BatchRunner(forced=False, pack_outputs=True) -> frames() (host synchronisation) -> synthesize_packed(mel[:total], lens) -> float32 D2H copy
  B  SpeechRunner (one captured graph: synthesis -> capacity vocoder -> int16 PCM) -> int16 D2H copy (capacity-sized: the host does not know the total)

Alternating legs, warmed, `--batches` per leg and `--repeats` repeats, in one process; every batch ends in a synchronise, so wall ms per batch is
the un-pipelined latency of one batch.  The batches cycle through `--distinct` different length tuples (a driver sees a new one every batch; A's
map cache holds four).  Also: the generator alone, capacity form vs exact form on identical rows, per-kernel times from the library's own
event timers (ProfScope), alternating -- the cost of the live word in the persistent block kernel against the exact form's run-to-run spread.

    python tools/speech_ab.py [--batch 64] [--batches 20] [--repeats 3] [--distinct 6]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o g -- python tools/speech_ab.py --alone 5     # the generator's kernels alone

Prints one JSON line per repeat and leg, then a summary line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fcl_taco2_amd  # noqa: E402,F401
from fcl_taco2_amd import _lib, engine, hparams as HP, ops, synthetic as SYN, vocoder as V  # noqa: E402
from fcl_taco2_amd.plan import SynthesisPlan  # noqa: E402

RATE = 22050.0


def main(argv=None, make_gen=None, blocks_prefix="pwg_layer"):
    """make_gen(device) -> generator: another generator family under the same protocol (tools/hifigan_ab.py --speech); blocks_prefix: the launch-record
    names summed as `blocks_ms` in the generator-alone comparison"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=6)
    ap.add_argument("--t-lo", type=int, default=60)
    ap.add_argument("--t-hi", type=int, default=100)
    ap.add_argument("--alone", type=int, default=0, metavar="N", help="only the generator alone, N alternating exact / capacity passes without the "
                    "library's timers: the run to put under `rocprofv3 --kernel-trace --stats` (pwg_layer_pkernel vs pwg_layer_cap_pkernel)")
    args = ap.parse_args(argv)
    dev = "cuda:0"
    B, T_cap = args.batch, (args.t_hi + 15) // 16 * 16
    hp = HP.student_hparams()
    plan = SynthesisPlan(SYN.positive_duration_head(SYN.closed_form_state_dict(HP.param_spec(hp))), hp, dev)
    if make_gen is not None:
        gen = make_gen(dev)
    else:
        gen = V.ParallelWaveGANGenerator(V.PWGPlan({k: SYN.closed_form_tensor("pwg." + k, tuple(s)) for k, s in V.param_spec().items()}, dev))
    hop = gen.plan.hop
    sets = [SYN.batch_c2(hp.idim, batch=B, t_lo=args.t_lo, t_hi=args.t_hi, seed=1234 + i)[0] for i in range(args.distinct)]
    maps = []
    for xs in sets:  # calibration: exact maps of the batches that will be fed
        _, _, inter = engine.run(plan, engine.prepare(plan, xs), ops.DROP_RNG, return_intermediates=True)
        maps.append(inter["maps"])
    caps = engine.Caps.for_batches(maps, slack_steps=2)
    live = [int(m.n_frames) for m in maps]
    stream = engine.shared_streams(dev, 1)[0]
    ra = engine.BatchRunner(plan, B, T_cap, caps, forced=False, stream=stream, seed=77, pack_outputs=True)
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    rb = engine.SpeechRunner(plan, gen, B, T_cap, caps, stream=stream, seed=77)
    torch.cuda.synchronize()
    runner_bytes = torch.cuda.memory_allocated() - m0
    host_f32 = torch.empty(caps.frames * hop, dtype=torch.float32, pin_memory=True)
    host_i16 = torch.empty(rb.synth.M, dtype=torch.int16, pin_memory=True)
    host_f0 = torch.empty(B + 1, dtype=torch.int32, pin_memory=True)
    host_st = torch.empty(1, dtype=torch.int32, pin_memory=True)

    def leg_a(i):
        xs = sets[i % len(sets)]
        t0 = time.perf_counter()
        ra.load(xs)
        ra.replay()
        t1 = time.perf_counter()
        lens = ra.frames()  # the host synchronisation in the middle of the batch
        t2 = time.perf_counter()
        total = sum(lens)
        with torch.cuda.stream(stream):
            _, flat = gen.synthesize_packed(ra.mel[:total], lens, seed=i, return_flat=True)
            host_f32[: total * hop].copy_(flat[: total * hop], non_blocking=True)
        t3 = time.perf_counter()
        stream.synchronize()
        return total * hop, (t1 - t0) + (t3 - t2)

    def leg_b(i):
        xs = sets[i % len(sets)]
        t0 = time.perf_counter()
        rb.load(xs)
        rb.replay()
        with torch.cuda.stream(stream):
            host_i16.copy_(rb.pcm, non_blocking=True)
            host_f0.copy_(rb._frames.utt_frame0[: B + 1], non_blocking=True)
            host_st.copy_(rb.status, non_blocking=True)
        t1 = time.perf_counter()
        stream.synchronize()
        assert int(host_st[0]) == 0, ops.status_message(int(host_st[0]))
        return int(host_f0[B]) * hop, t1 - t0

    if args.alone:
        ra.load(sets[0])
        ra.replay()
        lens = ra.frames()
        mel, f0, st = ra.mel.clone(), ra._frames.utt_frame0.clone(), torch.zeros(1, dtype=torch.int32, device=dev)
        for rep in range(args.alone):
            gen.synthesize_packed(mel[: sum(lens)], lens, seed=rep)
            rb.synth.run(mel, f0, st)
        torch.cuda.synchronize()
        print(json.dumps(dict(alone_passes=args.alone, frames=sum(lens), frames_cap=caps.frames)))
        return
    for i in range(len(sets)):  # warm-up: every length tuple once through both legs
        leg_a(i)
        leg_b(i)
    rows = []
    for rep in range(args.repeats):
        for name, leg in (("A", leg_a), ("B", leg_b)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            samples, enq = 0, 0.0
            for i in range(args.batches):
                s, e = leg(i)
                samples += s
                enq += e
            dt = time.perf_counter() - t0
            row = dict(leg=name, repeat=rep, ms_per_batch=1e3 * dt / args.batches, rtf=dt / (samples / RATE), enqueue_ms_per_batch=1e3 * enq / args.batches,
                       samples_per_batch=samples / args.batches)
            if name == "B":
                row["live_over_capacity"] = samples / args.batches / float(rb.synth.M)
            rows.append(row)
            print(json.dumps(row), flush=True)
    # ---- the generator alone on identical rows: exact form vs capacity form, per-kernel event times, alternating
    ra.load(sets[0])
    ra.replay()
    lens = ra.frames()
    total = sum(lens)
    mel = ra.mel.clone()
    f0 = ra._frames.utt_frame0.clone()
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    alone = {"exact": [], "capacity": []}
    for rep in range(5):
        for form in ("exact", "capacity"):
            _lib.prof_enable(True)
            if form == "exact":
                gen.synthesize_packed(mel[:total], lens, seed=rep)
            else:
                rb.synth.run(mel, f0, st)
            torch.cuda.synchronize()
            p = _lib.prof_collect()
            _lib.prof_enable(False)
            blocks = sum(v["ms"] for k, v in p.items() if k.startswith(blocks_prefix))
            alone[form].append(dict(blocks_ms=blocks, all_kernels_ms=sum(v["ms"] for v in p.values())))
    summ = lambda leg, key: [r[key] for r in rows if r["leg"] == leg]
    out = dict(batch=B, phonemes=[args.t_lo, args.t_hi], distinct_batches=len(sets), live_frames=live, frames_cap=caps.frames,
               speech_runner_bytes=runner_bytes, capacity_synth_bytes=rb.synth.nbytes, bytes_per_capacity_sample=rb.synth.nbytes / float(rb.synth.M),
               A_ms_per_batch=summ("A", "ms_per_batch"), B_ms_per_batch=summ("B", "ms_per_batch"), A_rtf=summ("A", "rtf"), B_rtf=summ("B", "rtf"),
               A_enqueue_ms=summ("A", "enqueue_ms_per_batch"), B_enqueue_ms=summ("B", "enqueue_ms_per_batch"),
               generator_alone_frames=total, exact_blocks_ms=[r["blocks_ms"] for r in alone["exact"]],
               capacity_blocks_ms=[r["blocks_ms"] for r in alone["capacity"]], exact_all_ms=[r["all_kernels_ms"] for r in alone["exact"]],
               capacity_all_ms=[r["all_kernels_ms"] for r in alone["capacity"]])
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
