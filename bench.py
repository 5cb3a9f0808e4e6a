#!/usr/bin/env python3
"""bench.py — mel-frames/sec of the FCL-taco2-S synthesis hot path on MI355X (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \\
        bench.py --gpus N --steps K --warmup W

A "step" is one pass of the hot path (encoder -> predictors -> per-phoneme-parallel decoder loop -> postnet)
over one synthetic LJSpeech-shape batch (32 utterances, 60..100 phonemes each, forced
durations clip(Poisson(10),1,50), ~25.6 k mel frames), inputs already resident in HBM (engine.prepare runs
before the clock starts), prenet dropout on in its production (on-device RNG) mode, fp32 arithmetic.
Utterances are independent, so N ranks run N independent batches (different seeds; weak scaling, no
data-path collective); the clock is barrier + synchronize on both sides, MAX over ranks; `value` is the
whole-job frames / that time.  Exactly K steps are timed (one region; --regions R repeats it, median).

A plain run sets up, warms up, times the K steps, writes the outputs of the last timed step (--dump-outputs)
and prints ONE JSON line.  --full adds what takes runs of its own: on rank 0 (N=1 only) the other feeds and
duration forms of the same workload (replay only, predicted durations, calibrated capacities, the decode
driver), the live roofline figures of the dominant kernel (HIP events on the launching stream, via
fcl_prof_*), a bounded CPU baseline (the oracle = this build's CPU restatement of the reference, "port"),
and two child runs (the KD step, the headline in exact fp32); the training and vocoder workloads likewise
keep their profiled update, one-rank RCCL leg and CPU baseline behind --full.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
# one hardware queue per in-flight pass (the HIP default of 4 makes a 4th stream share a queue); must be set
# before the HIP runtime initialises
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

PEAK_F32_MFMA_TFLOPS = 157.3  # MI355X_MICROARCH.md: v_mfma_f32_16x16x4_f32 dense peak (= fp32 vector peak)
PEAK_BF16_MFMA_TFLOPS = 2500.0  # MI355X_MICROARCH.md: bf16 MFMA dense peak (the pipe the bf16x3 kernels issue on)


def mfma_ceiling(amp=None):
    """(peak TFLOP/s in the unit `achieved` is quoted in, label) of the pipe the GEMM kernels of this process ISSUE on.  `achieved` counts algorithmic
    fp32-equivalent FLOPs (2 M N K).  Default mode: every product is three bf16 MFMAs (a_hi b_hi + a_hi b_lo + a_lo b_hi), so the ceiling is the
    bf16 dense peak / 3; --amp bf16: one bf16 MFMA per product; FCL_PRECISION=0: v_mfma_f32_16x16x4_f32, the fp32 matrix peak.  (Round-2 VERDICT:
    the fp32 matrix peak is NOT a ceiling for the bf16x3 kernels -- they do not run on that pipe.)"""
    if os.environ.get("FCL_PRECISION", "1") == "0":
        return PEAK_F32_MFMA_TFLOPS, "fp32 MFMA (v_mfma_f32_16x16x4_f32) dense peak"
    if amp:
        return PEAK_BF16_MFMA_TFLOPS, "bf16 MFMA dense peak, one MFMA per product (--amp bf16)"
    return PEAK_BF16_MFMA_TFLOPS / 3.0, "bf16 MFMA dense peak / 3: each fp32-equivalent product issues three bf16 MFMAs (bf16x3 split)"


_REAL_STDOUT = None


def quiet_stdout():
    """Everything libraries print on fd 1 (RCCL writes a version banner there when its first communicator comes up) goes to stderr; the ONE JSON
    line is written to the real stdout by emit()."""
    global _REAL_STDOUT
    if _REAL_STDOUT is None:
        sys.stdout.flush()
        _REAL_STDOUT = os.dup(1)
        os.dup2(2, 1)


RANKS = []  # sharding.verify_world's per-rank records (filled in main() once the process group is up)


def emit(obj):
    if RANKS:
        obj = dict(obj, ranks=list(RANKS))
    # key order of the ONE line: every scalar first (a reader that keeps only the head of the line sees the numbers), then roofline and
    # cpu_baseline, then the long tables; the same scalars once more as the LAST key (a reader that keeps only the tail sees them too)
    scal = {k: v for k, v in obj.items() if not isinstance(v, (dict, list))}
    first = ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data"]
    ordered = {k: obj[k] for k in first if k in obj}
    ordered.update({k: v for k, v in scal.items() if k not in ordered})
    for k in ("roofline", "cpu_baseline", "config"):
        if k in obj:
            ordered[k] = obj[k]
    ordered.update({k: v for k, v in obj.items() if k not in ordered})
    ordered["scalars"] = {k: v for k, v in scal.items() if isinstance(v, (int, float)) and not isinstance(v, bool)}
    obj = ordered
    line = (json.dumps(obj) + "\n").encode()
    sys.stdout.flush()
    if _REAL_STDOUT is None:
        os.write(1, line)
    else:
        os.write(_REAL_STDOUT, line)


DUMP_LIMIT_BYTES = 64 << 20  # --dump-outputs: all files together


def dump_outputs(dirname, arrays):
    """--dump-outputs: `arrays` (name -> array-like) as DIR/<name>.npy, float64 where the values are float64 or integers (exact), float32 otherwise.
    At most DUMP_LIMIT_BYTES in all: an array beyond what is left keeps a fixed seeded sample of its rows (sorted), whose indices go to
    DIR/<name>_rows.npy.  Returns {name: shape written}."""
    import numpy as np

    os.makedirs(dirname, exist_ok=True)
    conv = {}
    for name, a in arrays.items():
        a = np.asarray(a)
        conv[name] = a.astype(np.float64 if (a.dtype == np.float64 or a.dtype.kind in "iub") else np.float32)
    left, written = DUMP_LIMIT_BYTES - 2 * 4096 * len(conv), {}  # (room for the .npy headers)
    for name in sorted(conv, key=lambda k: conv[k].nbytes):  # the small arrays first: only the largest one can need a sample
        a = conv[name]
        if a.nbytes > left and a.ndim >= 1 and a.shape[0] > 1:
            row_bytes = a.nbytes // a.shape[0]
            k = max(1, min(a.shape[0], (left - 8 * a.shape[0]) // (row_bytes + 8)))
            rows = np.sort(np.random.RandomState(0).choice(a.shape[0], size=k, replace=False))
            np.save(os.path.join(dirname, name + "_rows.npy"), rows.astype(np.float64))
            left -= rows.nbytes
            a = a[rows]
        if a.nbytes > left:
            raise SystemExit("bench.py: --dump-outputs: %s does not fit in %d bytes" % (name, DUMP_LIMIT_BYTES))
        np.save(os.path.join(dirname, name + ".npy"), a)
        left -= a.nbytes
        written[name] = list(a.shape)
    return written


def timed_regions(one_region, barrier, regions):
    """`regions` repetitions of the timed region (each: barrier + synchronize, EXACTLY K steps, barrier + synchronize); returns the list of wall
    times.  The reported figure is their MEDIAN (median of >= 20 timed iterations after warm-up; one region of K steps is only ~10 ms)."""
    out = []
    for _ in range(regions):
        barrier()
        t0 = time.perf_counter()
        one_region()
        barrier()
        out.append(time.perf_counter() - t0)
    return out


def median(xs):
    xs = sorted(xs)
    n = len(xs)
    return xs[n // 2] if n % 2 else 0.5 * (xs[n // 2 - 1] + xs[n // 2])


def self_launch(args, argv):
    """`python bench.py --gpus N` with N > 1 and no torch.distributed environment: start the N ranks ourselves (one process per GPU under
    torch.distributed.run, rendezvous on 127.0.0.1) as a CHILD process and pass its output and exit code through.  Runs before this process has
    made any GPU call (the launcher itself never touches the GPU)."""
    import socket
    import subprocess

    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return subprocess.run(cmd, env=env).returncode


def dry_run_launch(args):
    """--dry-run-launch: the N-rank launch path without a GPU (gloo): every rank joins the process group, contributes a fake (time, frames) pair to
    the same MAX / SUM reductions the real run uses, and rank 0 prints the one JSON line.  CPU test of the launcher (tests/test_bench_launch_cpu.py)."""
    import torch.distributed as dist

    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import sharding

    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo")
    dt, frames = sharding.aggregate_throughput(1e-3 * (rank + 1), 1000.0 * (rank + 1), dist if world > 1 else None, "cpu")
    if rank == 0:
        print(json.dumps({"metric": "dry run of the launcher (no GPU work)", "dry_run": True, "n_gpus": world, "workload": args.workload,
                          "max_seconds": dt, "sum_frames": frames, "steps": args.steps, "warmup": args.warmup}))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return 0


def run_child(extra_args, env_extra, timeout):
    """One more bench.py as a child process (started BEFORE this process initialises the GPU); returns its parsed JSON line or {"error": ...}."""
    import subprocess

    cmd = [sys.executable, os.path.abspath(__file__)] + extra_args
    try:
        r = subprocess.run(cmd, env=dict(os.environ, **env_extra), capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        return {"error": "timeout after %d s" % timeout}
    for line in reversed(r.stdout.strip().splitlines()):
        if line.startswith("{"):
            try:
                return json.loads(line)
            except ValueError:
                break
    return {"error": "rc %d: %s" % (r.returncode, r.stderr.strip().splitlines()[-1] if r.stderr.strip() else "no output")}


def pmc_traffic(kernel, workload=""):
    """HBM-side bytes per launch of `kernel` from the committed rocprofv3 PMC summaries (profiles/*pmc_fetch_size.csv and
    *pmc_write_size.csv, separate --pmc passes of this same command): 2 x FETCH_SIZE (gfx950 counts 128-B requests as 64 B,
    MI355X_MICROARCH.md §HBM) + WRITE_SIZE, KiB -> bytes.  None when no profile of that kernel is committed.
    workload: "" = the synthesis profile (rN_pmc_fetch_size.csv), else the tag of the workload's pair (rN_pmc_<workload>_fetch_size.csv); the
    latest round's pair that holds the kernel is the one used."""
    import re
    import csv
    import glob

    def norm(n):
        """(base name, template args or None): bench labels are "gemm_kernel<2,2,1,2>/bf16x3" or "feat_prenet_kernel/bf16x3", rocprofv3 rows
        "fcl::gemm_kernel<2, 2, 1, 2>" or "fcl::feat_prenet_x3_kernel<8, 3, 8>"."""
        n = n.split("(")[0].replace(" ", "").replace("fcl::", "").replace("void", "")
        x3 = n.endswith("/bf16x3")
        n = n[: -len("/bf16x3")] if x3 else n
        base, _, targs = n.partition("<")
        if x3 and not targs and "_x3_" not in base:
            base = base.replace("_kernel", "_x3_kernel")
        return base, (targs.rstrip(">") or None)

    def same(a, b):
        (ba, ta), (bb, tb) = norm(a), norm(b)
        if ba != bb:
            return False
        if ta is None or tb is None:
            return True
        xa, xb = ta.split(","), tb.split(",")  # the profiler prints trailing template arguments (arithmetic mode) the bench label omits
        n = min(len(xa), len(xb))
        return xa[:n] == xb[:n]

    # per-workload summary pairs (rN_pmc_fetch_size.csv / rN_pmc_write_size.csv, rN_pmc_vocoder_fetch_size.csv / ...): this workload's pair of the
    # latest round that holds the kernel
    best = None
    want = "pmc_%s_fetch_size.csv" % workload if workload else "pmc_fetch_size.csv"
    paths = [p for p in glob.glob(os.path.join(ROOT, "profiles", "*pmc_*fetch_size.csv")) if os.path.basename(p).split("_", 1)[-1] == want]
    rnd = lambda p: int((re.match(r"r(\d+)_", os.path.basename(p)) or [0, 0])[1])
    for fpath in sorted(paths, key=rnd):
        wpath = fpath[: -len("fetch_size.csv")] + "write_size.csv"
        if not os.path.exists(wpath):
            continue
        pair = {}
        for tag, path in (("fetch", fpath), ("write", wpath)):
            with open(path) as f:
                rows = list(csv.reader(f))
            # rows: kernel, launches, KiB per launch; a family name (no template arguments) matches every instantiation: launch-weighted mean
            hits = [(float(r[1]), float(r[2])) for r in rows[2:] if len(r) >= 3 and same(r[0], kernel)]
            if hits:
                n = sum(h[0] for h in hits)
                pair[tag] = (sum(h[0] * h[1] for h in hits) / n, os.path.basename(path), n)
        if len(pair) == 2:
            best = pair
    vals = best or {}
    if len(vals) != 2:
        return None, None
    return (2.0 * vals["fetch"][0] + vals["write"][0]) * 1024.0, "%s + %s" % (vals["fetch"][1], vals["write"][1])


# ---- the BINDING resource of the tiled GEMM / Conv1d / LSTM-step loops (round 6) ---------------------------------------------------
# These loops are bound by what a compute unit can pull through its vector-memory path into LDS, not by the matrix pipe: tools/stream_probe.hip
# (profiles/r4_stream_probe.log) measured 35 B/clk per CU = 21.8 TB/s over the chip for LDS-DMA streaming out of L2 with nothing else going on.
# The library reports the bytes every launch moves that way (fcl_prof_entry_t.fill_bytes: workgroups x k-chunks x (A lines + W lines) x 128 B).
CU_FILL_CEILING_B_PER_CLK = 35.5  # tools/stream_probe.hip: 21.8 TB/s / 256 CUs / 2.4 GHz
N_CUS, CLOCK_HZ = 256, 2.4e9     # MI355X_MICROARCH.md (max clock: a kernel that runs below it shows a LOWER delivered rate, never a higher one)


def pmc_lds_active(kernel, workload=""):
    """(SQ_LDS_IDX_ACTIVE / SQ_BUSY_CYCLES of `kernel`, source file) from the newest committed profiles/rN_pmc[_workload]_sq_counters.csv holding it."""
    import csv
    import glob
    import re

    want = "pmc_%s_sq_counters.csv" % workload if workload else "pmc_sq_counters.csv"
    rnd = lambda p_: int((re.match(r"r(\d+)_", os.path.basename(p_)) or [0, 0])[1])
    base = lambda n: n.split("(")[0].replace(" ", "").replace("fcl::", "").replace("void", "").split("/")[0]
    want_b, want_t = (base(kernel).split("<") + [""])[:2]
    for path in sorted([p_ for p_ in glob.glob(os.path.join(ROOT, "profiles", "*" + want)) if os.path.basename(p_).split("_", 1)[-1] == want], key=rnd, reverse=True):
        with open(path) as f:
            rows = list(csv.DictReader(f))
        hits = []
        for r in rows:
            b_, t_ = (base(r["kernel"]).split("<") + [""])[:2]
            xa, xb = want_t.rstrip(">").split(","), t_.rstrip(">").split(",")
            if b_ == want_b and (not want_t or xa == xb[: len(xa)]):
                hits.append(r)
        if hits:
            busy = sum(float(r["mean_SQ_BUSY_CYCLES"]) * float(r["launches"]) for r in hits)
            lds = sum(float(r["mean_SQ_LDS_IDX_ACTIVE"]) * float(r["launches"]) for r in hits)
            if busy > 0:
                return lds / busy, os.path.basename(path)
    return None, None


def binding_record(name, ms, fill_bytes, workload=""):
    """What the loop of a GEMM-class kernel is bound by: bytes delivered into LDS per clock and CU over the launch's whole duration (prologue and epilogue
    included: a lower bound of the main loop's rate) against the measured per-CU ceiling, and the fraction of busy cycles the LDS array was active."""
    if not fill_bytes or ms <= 0:
        return None
    rate = fill_bytes / (ms * 1e-3) / N_CUS / CLOCK_HZ
    lds, src = pmc_lds_active(name, workload)
    return {"resource": "per-CU global->LDS delivery (LDS-DMA)", "achieved_B_per_clk_per_cu": rate, "ceiling_B_per_clk_per_cu": CU_FILL_CEILING_B_PER_CLK,
            "frac": rate / CU_FILL_CEILING_B_PER_CLK, "fill_bytes_per_launch_sum": fill_bytes, "chip_TB_per_s": fill_bytes / (ms * 1e-3) / 1e12,
            "lds_idx_active_over_sq_busy": lds, "lds_counter_source": src,
            "note": "fill bytes = workgroups x 32-k chunks x (A + W lines) x 128 B as launched (fcl_prof_entry_t.fill_bytes) / HIP-event duration of the whole launch / "
                    "256 CUs / 2.4 GHz; ceiling = tools/stream_probe.hip (21.8 TB/s chip-wide, profiles/r4_stream_probe.log); lds_idx_active_over_sq_busy = "
                    "SQ_LDS_IDX_ACTIVE / SQ_BUSY_CYCLES from the committed PMC pass"}


def e2e_workload(args, rank, world, dev, dist):
    """BASELINE configs[4]: phoneme -> waveform, FCL-taco2-S (forced durations, as in the headline workload) + the Parallel WaveGAN generator, batch 64;
    `--workload vocoder` times the generator alone on the same mels.  value = real-time factor = wall seconds per second of audio (22 050 Hz, hop 256)."""
    import numpy as np
    import torch

    from fcl_taco2_amd import _lib, engine, hparams as HP, ops, sharding, synthetic as SYN, vocoder as V
    from fcl_taco2_amd.plan import SynthesisPlan

    e2e = args.workload == "tts_e2e"
    B = 64 if args.batch == 32 else args.batch  # configs[4] is quoted on batch 64
    hp = HP.student_hparams()
    sd_np = SYN.closed_form_state_dict(HP.param_spec(hp))
    plan = SynthesisPlan(sd_np, hp, dev)
    xs, ds = SYN.batch_c2(hp.idim, batch=B, seed=1234 + rank)
    prep = engine.prepare(plan, xs, ds)
    vsd = {k: SYN.closed_form_tensor("pwg." + k, tuple(shp)) for k, shp in V.param_spec().items()}
    gen = V.ParallelWaveGANGenerator(V.PWGPlan(vsd, dev))
    runner = engine.GraphRunner(plan, prep, seed=77)
    mel = runner.replay()
    lens = [int(n) for n in runner.utt_frames]
    frames = int(sum(lens))
    samples = frames * gen.plan.hop
    audio_s = samples / 22050.0

    def step(i):
        with torch.cuda.stream(runner.stream):
            m = runner.replay() if e2e else mel
            return gen.synthesize_packed(m, lens, seed=i)

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    for i in range(args.warmup):
        step(i)
    barrier()
    t0 = time.perf_counter()
    for i in range(args.steps):
        wavs = step(1000 + i)
    barrier()
    dt = time.perf_counter() - t0
    dt, samples_all = sharding.aggregate_throughput(dt, samples, dist, dev)
    rtf = (dt / args.steps) / (samples_all / world / 22050.0)
    out = {
        "metric": ("phoneme -> waveform real-time factor (FCL-taco2-S + Parallel WaveGAN, batch=%d)" if e2e else
                   "mel -> waveform real-time factor (Parallel WaveGAN generator, batch=%d)") % B,
        "value": rtf, "unit": "wall s / audio s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps,
        "higher_is_better": False, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32 via bf16x3-split MFMA operands, fp32 accumulate", "data": "synthetic",
        "samples_per_s": samples_all * args.steps / dt, "x_real_time": 1.0 / rtf,
        "config": {"workload": "BASELINE configs[4]: %d utterances/GPU, %d mel frames = %.0f s of audio per batch; synthesis as in configs[1] (forced durations, "
                               "hipGraph replay)%s; generator = published ParallelWaveGAN v1 (30 layers, 64/128 channels, hop 256), closed-form weights, "
                               "device noise" % (B, frames, audio_s, "" if e2e else " OUTSIDE the timed region"),
                   "parallelism": "%d independent replicas (utterance-sharded, no collective)" % world},
    }
    if args.dump_outputs and rank == 0:  # the waveforms of the last timed step, utterances back to back (lengths: frames x hop)
        out["dumped"] = dump_outputs(args.dump_outputs, {"wav": torch.cat([w.reshape(-1) for w in wavs]).cpu().numpy(), "utt_frames": np.asarray(lens)})
    if args.full and rank == 0 and world == 1:
        # ---- live roofline of the dominant kernel (the fused residual block): HBM bytes it must move per launch / its HIP-event duration
        torch.cuda.synchronize()
        _lib.prof_enable(True)
        gen.synthesize_packed(mel, lens, seed=5)
        torch.cuda.synchronize()
        prof = _lib.prof_collect()
        _lib.prof_enable(False)
        dom = max(prof, key=lambda k: prof[k]["ms"])
        d = prof[dom]
        # algorithmic bytes per sample and layer: x planes in 256 + out 256, skips fp32 read + write 512, and the auxiliary term: one 128-byte
        # coefficient line (frame-rate form, default) or 384 bytes of upsampled-feature planes (96 padded columns, hi | lo)
        aux_b = 128 if V.aux_frame_rate(gen.plan) else 384
        bytes_per_launch = (1024.0 + aux_b) * samples
        achieved = bytes_per_launch * d["launches"] / (d["ms"] * 1e-3) / 1e9
        traffic, src = pmc_traffic(dom, "vocoder")
        out["roofline"] = {"bound": "hbm", "kernel": dom, "achieved": achieved, "peak": 8000.0, "unit": "GB/s", "frac": achieved / 8000.0,
                           "traffic": traffic, "traffic_source": src, "avg_launch_us": 1e3 * d["ms"] / d["launches"], "launches_per_step": d["launches"],
                           "bytes_per_launch": bytes_per_launch, "share_of_kernel_time": d["ms"] / sum(v["ms"] for v in prof.values()),
                           "fp32_equivalent_tflops": d["flops"] / (d["ms"] * 1e-3) / 1e12,
                           "note": "algorithmic %d B per sample per residual block (x planes 256 in + 256 out, skip accumulator 512, auxiliary term %d: %s); "
                                   "the block's 86 kFLOP per sample put it on the HBM side of the fp32-equivalent ridge"
                                   % (1024 + aux_b, aux_b, "coefficient line of the frame-rate form" if aux_b == 128 else "planes of the upsampled features")}
        if not args.no_cpu_baseline:
            from oracle import fcl_oracle as O, pwg_oracle as PO

            try:
                avail = len(os.sched_getaffinity(0))
            except AttributeError:
                avail = os.cpu_count() or 1
            torch.set_num_threads(max(1, min(avail, args.cpu_threads)))
            sd = {k: torch.from_numpy(np.asarray(v)) for k, v in sd_np.items()}
            tv = {k: torch.from_numpy(v) for k, v in vsd.items()}
            with torch.no_grad():
                t1 = time.perf_counter()
                cmel = O.inference(sd, hp, torch.from_numpy(xs[0]), dur=torch.from_numpy(ds[0]), prenet_keep="rng")["after"]
                t_mel = time.perf_counter() - t1
                nf = min(48, cmel.shape[0])
                PO.inference(tv, cmel[:8].numpy())  # warm-up
                t1 = time.perf_counter()
                PO.inference(tv, cmel[:nf].numpy())
                t_voc = (time.perf_counter() - t1) * cmel.shape[0] / nf
            a_s = cmel.shape[0] * 256 / 22050.0
            out["cpu_baseline"] = {"value": ((t_mel if e2e else 0.0) + t_voc) / a_s, "unit": "wall s / audio s", "cores": torch.get_num_threads(), "kind": "port",
                                   "sample": "utterance 0 (%d frames): %s the generator through oracle/pwg_oracle.py on its first %d frames, scaled to the utterance "
                                             "(%.1f s)" % (cmel.shape[0], "mel through oracle/fcl_oracle.py (%.2f s) +" % t_mel if e2e else "", nf, t_voc)}
    del wavs
    return out


def forward_tf_workload(args, rank, world, dev, dist, batch, frames, S, T):
    """the student's teacher-forced `forward()` under eval() + no_grad() (what the reference's CustomEvaluator runs every epoch,
    tts_distill.py:91-111): H1-H12 incl. the distillation terms against a teacher 5-tuple computed once, outside the timed region."""
    import torch

    from fcl_taco2_amd import sharding, synthetic as SYN
    from fcl_taco2_amd.training import TrainEngine

    teng = TrainEngine(SYN.build_model("kd_teacher", T, None, dev))
    know = teng.knowledge(batch, mode="train")
    model = SYN.build_model("student", S, T, dev)
    model.eval()
    kw = {k: v for k, v in batch.items() if not k.startswith("_")}

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    with torch.no_grad():
        for _ in range(args.warmup):
            loss = model(teacher_knowledge=know, **kw)
        barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            loss = model(teacher_knowledge=know, **kw)
        barrier()
        dt = time.perf_counter() - t0
    dt, frames_all = sharding.aggregate_throughput(dt, frames, dist, dev)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"loss": [float(loss)]})
    return {
        "metric": "mel-frames/sec (FCL-taco2-S teacher-forced forward(), eval + no_grad, batch=%d, 80-mel)" % args.batch,
        "value": frames_all * args.steps / dt, "unit": "mel-frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32 (GEMMs on bf16x3-split MFMA operands, fp32 accumulate; FCL_PRECISION=0 = exact fp32 MFMA)", "data": "synthetic", "loss": float(loss),
        "config": {"workload": "SURVEY §8d C2(ii): %d utterances/GPU, %d frames/GPU-batch, ys ~ N(0,1), named losses incl. the four distillation terms "
                               "against a resident teacher 5-tuple, eager launches (shapes change per batch)" % (args.batch, frames),
                   "parallelism": "%d independent replicas (utterance-sharded, no collective)" % world},
    }


def train_workload(args, rank, world, dev, dist):
    """KD step (frozen train-mode FCL-taco2-T forward -> FCL-taco2-S forward / backward / all-reduce / clip / Adam, tts_distill.py:143-182) or the
    teacher's own training step (tts.py:137-179), train-form regularisers, masks drawn on the device.  One process per GPU; gradients are
    averaged over ranks in buckets overlapped with backward (RCCL).  `value` = ms per step (MAX over ranks)."""
    import numpy as np
    import torch

    from fcl_taco2_amd import hparams as HP, sharding, synthetic as SYN
    from fcl_taco2_amd.converter import CustomConverter
    from fcl_taco2_amd.training import TrainEngine

    torch.set_num_threads(4)  # the step is ~1000 launches from this thread; a 256-thread intra-op pool spinning after small CPU ops slows them (train.py)
    S, T = HP.student_hparams(), HP.teacher_hparams()
    kd = args.workload == "kd_step"
    B = args.batch if (kd or args.batch != 32 or args.workload == "forward_tf") else 16  # shipped recipes: 32 / GPU for KD, 16 / GPU for the teacher
    xs, ys, ds, f0, en = SYN.training_batch(80, S.idim, batch=B, t_lo=60, t_hi=100, seed=1234 + rank, zero_frac=0.03, lam=10.0, hi=50)
    batch = CustomConverter(1, True, True)([(xs, ys, None, ds, f0, en)])
    frames = int(sum(y.shape[0] for y in ys))
    for k in ("xs", "ys", "extras", "f0", "energy"):  # inputs resident in HBM when the timed region starts; the integer layout tensors stay on the host
        batch[k] = batch[k].to(dev)
    if args.workload == "forward_tf":
        return forward_tf_workload(args, rank, world, dev, dist, batch, frames, S, T)
    amp = None if args.amp == "none" else args.amp
    teng = TrainEngine(SYN.build_model("kd_teacher", T, None, dev), amp=amp) if kd else None
    eng = TrainEngine(SYN.build_model("student", S, T, dev) if kd else SYN.build_model("teacher", T, None, dev), seed=rank, amp=amp)

    from fcl_taco2_amd.training import KDPipeline

    # a second batch object with the same content: the pipeline keys its look-ahead on the batch identity, as a data loader would present it
    batches = [batch, dict(batch)]
    pipe = KDPipeline(teng, eng) if (kd and not args.no_overlap) else None
    counter = [0]

    def step():
        i = counter[0]
        counter[0] += 1
        if pipe is not None:  # teacher of step i+1 overlaps the student update of step i
            return pipe.step(batches[i % 2], batches[(i + 1) % 2])
        know = teng.knowledge(batch, mode="train") if kd else None
        return eng.train_step(batch, know, mode="train")

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    steps, warmup = args.steps, args.warmup
    for _ in range(warmup):
        rep = step()
    last = [rep]

    def region():
        for _ in range(steps):
            last[0] = step()

    agg = [sharding.aggregate_throughput(t, frames, dist, dev) for t in timed_regions(region, barrier, max(1, args.regions))]
    rep = last[0]
    if args.dump_outputs and rank == 0:  # what the update hands its caller: the named losses and the gradient norm of the last timed step
        sc = {}
        for k, v in rep.items():
            v = v() if callable(v) else v
            v = v.item() if torch.is_tensor(v) and v.numel() == 1 else v
            if isinstance(v, (int, float)) and not isinstance(v, bool):
                sc[k] = [float(v)]
        dump_outputs(args.dump_outputs, sc)
    dts = [a[0] for a in agg]
    dt, frames_all = median(dts), agg[0][1]
    ms = 1e3 * dt / steps
    # algorithmic FLOPs per frame per step: KD = teacher fwd 42.3 + 3 x (student 4.29 + projections 1.89) = 61 MFLOP; teacher = 3 x 42.3
    mflop = 61.0 if kd else 127.0
    achieved = mflop * 1e6 * frames / (dt / steps) / 1e12
    peak, peak_note = mfma_ceiling(amp)
    # ---- dominant kernel of the step: HIP events around every launch of ONE more update (single stream order per stream; the events serialise nothing
    # but add host time, so this update is not part of the timed regions), grouped per kernel family as in the synthesis leg
    dom_roof, launches_per_step, host_ms = None, None, None
    if args.full and rank == 0 and world == 1:
        from fcl_taco2_amd import _lib

        torch.cuda.synchronize()
        t_h = time.perf_counter()
        step()
        host_ms = 1e3 * (time.perf_counter() - t_h)  # host time to ENQUEUE one update (returns before the GPU finishes)
        torch.cuda.synchronize()
        _lib.prof_enable(True)
        step()
        torch.cuda.synchronize()
        prof = _lib.prof_collect()
        _lib.prof_enable(False)
        fam = {}
        for k, v in prof.items():
            f = fam.setdefault(k.split("<")[0].split("/")[0], {"ms": 0.0, "launches": 0, "flops": 0.0, "fill_bytes": 0.0, "members": []})
            f["ms"] += v["ms"]; f["launches"] += v["launches"]; f["flops"] += v["flops"]; f["fill_bytes"] += v.get("fill_bytes", 0.0); f["members"].append(k)
        gemm_fams = {k: v for k, v in fam.items() if v["flops"] > 0}
        if gemm_fams:
            dname = max(gemm_fams, key=lambda k: gemm_fams[k]["ms"])
            d = gemm_fams[dname]
            ach = d["flops"] / (d["ms"] * 1e-3) / 1e12
            traffic, tsrc = pmc_traffic(dname, args.workload)
            dom_roof = {"bound": "mfma", "kernel": dname, "instantiations": sorted(d["members"]), "achieved": ach, "peak": peak, "unit": "TFLOP/s",
                        "frac": ach / peak, "traffic": traffic, "traffic_source": tsrc, "avg_launch_us": 1e3 * d["ms"] / d["launches"],
                        "launches_per_step": d["launches"], "flops_per_launch": d["flops"] / d["launches"],
                        "share_of_profiled_kernel_time": d["ms"] / (sum(v["ms"] for v in fam.values()) or 1.0), "peak_is": peak_note,
                        "note": "achieved = algorithmic fp32-equivalent FLOPs (2*M*N*K) of this kernel family's launches in one update / their "
                                "HIP-event durations; only the library's GEMM-class launches carry profile scopes"}
            dom_roof["binding"] = binding_record(dname, d["ms"], d["fill_bytes"], args.workload)
            dom_roof["kernels"] = {}
            for k, v in sorted(fam.items(), key=lambda kv: -kv[1]["ms"]):
                if v["flops"] <= 0:
                    continue
                e = {"ms_per_step": v["ms"], "launches_per_step": v["launches"], "tflops": v["flops"] / (v["ms"] * 1e-3) / 1e12, "mfma_frac": v["flops"] / (v["ms"] * 1e-3) / 1e12 / peak}
                b_ = binding_record(k, v["ms"], v["fill_bytes"], args.workload)
                if b_:
                    e["binding"] = {kk: b_[kk] for kk in ("achieved_B_per_clk_per_cu", "frac", "lds_idx_active_over_sq_busy")}
                dom_roof["kernels"][k] = e
        launches_per_step = int(sum(v["launches"] for v in prof.values()))
    # ---- the same update on the schedule a rank of an N-GPU job runs (VERDICT r3 #5c): a ONE-rank RCCL group, every bucket's
    # all_reduce(AVG, async_op=True) issued from the weight-gradient stream while backward continues, waited for in optimizer_step()
    dp_sched = None
    if args.full and rank == 0 and world == 1 and not args.no_dp_schedule:
        try:
            import socket

            import torch.distributed as dist1

            from fcl_taco2_amd.training import GradBuckets

            sk = socket.socket()
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
            sk.close()
            dist1.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1, device_id=torch.device(dev))
            eng.buckets = GradBuckets(eng.gflat, eng.buckets.bounds, None, force=True)
            for _ in range(max(2, warmup, GradBuckets.TRIAL_TOTAL + 1)):  # (the placement trial completes before the clock starts)
                step()
            dts_dp = timed_regions(region, lambda: torch.cuda.synchronize(), max(3, args.regions // 2))
            dp_sched = {"ms_per_step": 1e3 * median(dts_dp) / steps, "collectives_issued": eng.buckets.collectives, "inline": eng.buckets.inline,
                        "policy": eng.buckets.schedule(),
                        "note": "one-rank RCCL process group, FCL_DP_FORCE_COLLECTIVE schedule: 4 bucketed all_reduce(AVG, async) per update issued from the "
                                "weight-gradient stream (identity result); what a rank of an N-GPU job enqueues, minus the wire time"}
            eng.buckets = GradBuckets(eng.gflat, eng.buckets.bounds, None, force=False)
            dist1.destroy_process_group()
        except Exception as e:  # reported, never fatal: the headline figure above is already measured
            dp_sched = {"error": repr(e)}
    name = "KD step" if kd else "teacher training step"
    cpu = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        # ---- CPU baseline ("port"): the same update through the oracle's differentiable restatement + torch autograd + torch.optim.Adam on a bounded
        # sample (the first 2 utterances of the batch; the reference's own 32-utterance CPU step took ~38 s in the survey container)
        from oracle import fcl_oracle as O

        try:
            avail = len(os.sched_getaffinity(0))
        except AttributeError:
            avail = os.cpu_count() or 1
        torch.set_num_threads(max(1, min(avail, args.cpu_threads)))
        n = 2
        sb = O.convert_batch(xs[:n], ys[:n], ds[:n], f0[:n], en[:n])
        sframes = int(sum(y.shape[0] for y in ys[:n]))
        f = lambda spec: {k: torch.from_numpy(np.asarray(v)) for k, v in SYN.closed_form_state_dict(spec).items()}
        if kd:
            tsd = f(HP.param_spec(T))
            ssd = {k: (v.requires_grad_(True) if v.dtype.is_floating_point and "running" not in k else v) for k, v in f(HP.param_spec(S, T, True)).items()}
        else:
            ssd = {k: (v.requires_grad_(True) if v.dtype.is_floating_point and "running" not in k else v) for k, v in f(HP.param_spec(T)).items()}
        params = [v for v in ssd.values() if v.dtype.is_floating_point and v.requires_grad]
        opt = torch.optim.Adam(params, lr=1e-3, eps=1e-6)

        def cpu_step():
            opt.zero_grad()
            if kd:
                with torch.no_grad():
                    know = O.model_forward(tsd, T, sb, "kd_teacher", bn_train=True)
                out = O.model_forward(ssd, S, sb, "student", T, True, know, bn_train=True)
            else:
                out = O.model_forward(ssd, T, sb, "teacher", bn_train=True)
            out["loss"].backward()
            torch.nn.utils.clip_grad_norm_(params, 1.0)
            opt.step()

        cpu_step()
        t1, reps = time.perf_counter(), 0
        while time.perf_counter() - t1 < args.cpu_seconds and reps < 20:
            cpu_step()
            reps += 1
        cdt = (time.perf_counter() - t1) / max(reps, 1)
        cpu = {"value": 1e3 * cdt * frames / sframes, "unit": "ms/step (scaled to the full batch by frames)", "cores": torch.get_num_threads(), "kind": "port",
               "frames_per_s": sframes / cdt,
               "sample": "%d updates on the first %d utterances (%d frames) of the batch through oracle/fcl_oracle.py + torch autograd + torch.optim.Adam "
                         "(torch %s CPU fp32, batch-statistics BatchNorm, dropout off), %.2f s each" % (reps, n, sframes, torch.__version__, cdt)}
    out = {
        "metric": "%s time (ms) (%s, batch=%d/GPU, 80-mel)" % (name, "FCL-taco2-T frozen teacher fwd + FCL-taco2-S fwd/bwd/Adam" if kd else "FCL-taco2-T fwd/bwd/Adam", B),
        "value": ms, "unit": "ms/step", "n_gpus": world, "steps": steps, "warmup": warmup, "ms_per_step": ms, "higher_is_better": False, "scaling": "weak",
        "vs_baseline": None, "dtype": ("bf16 GEMM operands (rounded), fp32 accumulate / master weights / norms / losses / Adam (--amp bf16)" if amp else
                                       "f32 (GEMMs on bf16x3-split MFMA operands, fp32 accumulate; FCL_PRECISION=0 = exact fp32 MFMA)"), "data": "synthetic",
        "frames_per_s": frames_all * steps / dt, "loss": rep["loss"], "grad_norm": rep["grad_norm"],
        "config": {"workload": "SURVEY §8d %s: %d utterances/GPU, 60-100 phonemes, durations clip(Poisson(10),1,50) with 3%% zero-duration phonemes, "
                               "%d frames/GPU-batch, train-form BatchNorm / dropout / zoneout (device RNG), Adam lr 1e-3 eps 1e-6, clip 1.0, "
                               "closed-form weights" % ("C3" if kd else "C4", B, frames),
                   "parallelism": "dp%d: one process per GPU, gradient all-reduce (AVG) in 4 buckets overlapped with backward" % world,
                   "pipeline": ("frozen teacher one batch ahead on a second HIP stream (steady-state time per update)" if pipe is not None else
                                "teacher forward and update back to back on one stream"),
                   "stream_placement": {"weight_gradient_stream": {1: "moved off the main stream's compute pipe", 0: "apart as created", -1: "contends, could not be placed"}.get(
                                            getattr(eng.native, "side_moved", 0), "unplaced") if eng.native is not None else "per-launch engine",
                                        "frozen_teacher_stream": ("measured apart from the student's two streams" if getattr(pipe.side, "fcl_placed", False) else "as created")
                                        if pipe is not None else None}},
        "timing": {"statistic": "median over %d timed regions of exactly %d steps each (barrier + synchronize on both sides; MAX over ranks per region)"
                                % (len(dts), steps), "region_ms": [round(1e3 * t, 3) for t in dts], "best_ms_per_step": 1e3 * min(dts) / steps},
        "whole_step": {"achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak, "peak_is": peak_note,
                       "achieved_vs_fp32_matrix_peak": achieved / PEAK_F32_MFMA_TFLOPS,
                       "note": "algorithmic %.0f MFLOP per frame per step (SURVEY.md §8d) x frames / measured step time (per GPU)" % mflop},
    }
    out["roofline"] = dom_roof if dom_roof is not None else dict(out["whole_step"], bound="mfma", kernel="whole step", traffic=None)
    if dp_sched is not None:
        out["dp_schedule"] = dp_sched
    if launches_per_step is not None:
        out["profiled_gemm_launches_per_step"], out["host_enqueue_ms"] = launches_per_step, host_ms
    # launches of one update as the native engines count them (fcl_te_last_launches: every kernel / memset / copy they enqueue; Adam + norm on top)
    try:
        n_l = eng.native.launches() + (teng.native.launches() if (kd and teng.native is not None) else 0)
        out["launches_per_update"] = {"student_or_teacher_engine": eng.native.launches(), "frozen_teacher_forward": teng.native.launches() if kd else 0, "sum": n_l}
    except AttributeError:
        pass
    if cpu is not None:
        out["cpu_baseline"] = cpu
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--model", choices=["student", "teacher"], default="student")
    ap.add_argument("--workload", choices=["synthesis", "kd_step", "teacher_step", "forward_tf", "tts_e2e", "vocoder"], default="synthesis",
                    help="synthesis = BASELINE.json's headline metric (default); kd_step / teacher_step = the training step (SURVEY.md §8d C3/C4)")
    ap.add_argument("--amp", choices=["none", "bf16"], default="none", help="kd_step / teacher_step: the mixed-precision variant (bf16-rounded GEMM operands, "
                    "fp32 accumulate / master weights / optimizer) of the reference's --use-amp recipes")
    ap.add_argument("--streams", type=int, default=4, help="batches in flight per GPU (independent passes on separate HIP streams)")
    ap.add_argument("--feed", choices=["fresh", "replay"], default="fresh", help="synthesis: fresh = every pass takes a NEW batch through host packing + "
                    "one capacity graph (first node: the H2D pull of the packed block; device-built row maps) -- what inference() times; replay = one prepared batch "
                    "(host-built maps, outside the clock) replayed from a hipGraph (rounds 1-2)")
    ap.add_argument("--batches", type=int, default=4, help="synthesis: distinct synthetic batches fed round-robin")
    ap.add_argument("--cap-slack", type=int, default=0, help="synthesis: decoder steps of the capacity graph beyond the longest duration of the batches it serves (each costs three launches that exit at once)")
    ap.add_argument("--eager", action="store_true", help="launch kernel by kernel instead of replaying captured hipGraphs")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-dp-schedule", action="store_true", help="kd_step / teacher_step: skip the one-rank RCCL leg (the N-GPU schedule on one GPU)")
    ap.add_argument("--no-overlap", action="store_true", help="kd_step: run teacher forward and student update back to back on one stream")
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="target CPU time of the bounded baseline sample")
    ap.add_argument("--regions", type=int, default=1, help="repetitions of the timed region (each EXACTLY --steps steps between barrier + synchronize); "
                    "value / ms_per_step are the MEDIAN region (default 1: the timed steps are exactly --steps)")
    ap.add_argument("--full", action="store_true", help="also measure what takes runs of its own: other feeds and duration forms, the decode driver, "
                    "roofline and per-kernel figures, CPU baselines, the one-rank RCCL leg, and (synthesis, 1 GPU) the two child runs "
                    "(kd_step_ms + its CPU baseline; value_fp32_exact under FCL_PRECISION=0)")
    ap.add_argument("--no-extras", action="store_true", help="with --full, synthesis, 1 GPU: skip the two child runs")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the timed path computed in its last step as DIR/<name>.npy "
                    "(float32 / float64, at most 64 MB in all); the inputs are seeded, so runs with the same arguments see the same inputs")
    ap.add_argument("--dry-run-launch", action="store_true", help="exercise the N-rank launch path on CPU (gloo), no GPU work")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:  # the driver's form `python bench.py --gpus N`: launch the ranks ourselves
        raise SystemExit(self_launch(args, sys.argv[1:]))
    if args.dry_run_launch:
        raise SystemExit(dry_run_launch(args))

    quiet_stdout()
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d" % (args.gpus, world))

    if rank == 0 and not os.path.exists(os.path.join(ROOT, "fcl-taco2_amd", "libfcl_hip.so")):  # hipcc only: no GPU call
        import __graft_entry__ as ge0

        ge0.build()
    # ---- --full: numbers that ride on the line, measured in CHILD processes started before this one touches the GPU: the second north-star number
    # (student-KD step time, with its own CPU baseline) and the headline metric in exact-fp32 arithmetic (FCL_PRECISION is read once per process).
    # The children run --full themselves and keep the median of 11 timed regions these two figures have always been quoted as.
    extras = {}
    if args.full and args.workload == "synthesis" and world == 1 and not args.no_extras:
        common = ["--steps", str(args.steps), "--warmup", str(args.warmup), "--regions", "11", "--full", "--no-extras"]
        kd = run_child(["--workload", "kd_step", "--cpu-threads", str(args.cpu_threads)] + common + (["--no-cpu-baseline"] if args.no_cpu_baseline else []),
                       {}, 900)
        extras["kd_step"] = ({k: kd.get(k) for k in ("metric", "value", "unit", "ms_per_step", "steps", "frames_per_s", "dtype", "roofline", "cpu_baseline",
                                                      "timing", "whole_step", "profiled_gemm_launches_per_step", "host_enqueue_ms", "dp_schedule", "config")} if "error" not in kd else kd)
        fx = run_child(["--workload", "synthesis", "--model", args.model, "--batch", str(args.batch), "--streams", str(args.streams), "--no-cpu-baseline"]
                       + common, {"FCL_PRECISION": "0"}, 600)
        extras["fp32_exact"] = ({k: fx.get(k) for k in ("value", "unit", "ms_per_step", "dtype", "roofline", "timing")} if "error" not in fx else fx)

    import numpy as np
    import torch

    assert torch.cuda.is_available(), "bench.py needs a GPU (the product path has no CPU fallback)"
    torch.set_num_threads(4)  # launches are issued from this thread: keep torch's 256-thread intra-op pool from spinning next to it
    torch.cuda.set_device(local_rank)
    dev = "cuda:%d" % local_rank
    dist = None
    if world > 1:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=torch.device(dev))
    import __graft_entry__ as ge

    ge.build() if rank == 0 and not os.path.exists(os.path.join(ROOT, "fcl-taco2_amd", "libfcl_hip.so")) else None
    if dist is not None:
        dist.barrier()
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import _lib, engine, hparams as HP, ops, synthetic as SYN
    from fcl_taco2_amd.plan import SynthesisPlan

    # every rank: the RCCL communicator's size as seen here must be --gpus and an all-reduce of ones on the device must return it (raises
    # otherwise); one line per rank on stderr, the gathered records on rank 0's JSON line ("ranks")
    from fcl_taco2_amd import sharding as _sh

    RANKS[:] = _sh.verify_world(dist, args.gpus, dev)
    print("bench.py rank %d/%d on %s: communicator size %d, all-reduce of ones = %g" % (
        rank, world, dev, RANKS[rank]["world_size_seen"], RANKS[rank]["allreduce_of_ones"]), file=sys.stderr, flush=True)

    if args.workload in ("tts_e2e", "vocoder"):
        out = e2e_workload(args, rank, world, dev, dist)
        if rank == 0:
            emit(out)
        if dist is not None:
            dist.destroy_process_group()
        return
    if args.workload != "synthesis":
        out = train_workload(args, rank, world, dev, dist)
        if rank == 0:
            emit(out)
        if dist is not None:
            dist.destroy_process_group()
        return
    hp = HP.student_hparams() if args.model == "student" else HP.teacher_hparams()
    sd_np = SYN.closed_form_state_dict(HP.param_spec(hp))
    plan = SynthesisPlan(sd_np, hp, dev)
    # ---- the workload: `--batches` different synthetic batches of the configs[1] shape (other phoneme counts and durations each), fed round-robin;
    # the first one is the batch the roofline / CPU-baseline legs use
    T_CAP = 100
    batches = [SYN.batch_c2(hp.idim, batch=args.batch, t_hi=T_CAP, seed=1234 + rank + 1000 * j) for j in range(max(1, args.batches))]
    xs, ds = batches[0]
    bframes = [int(sum(int(d.sum()) for d in b[1])) for b in batches]
    frames = bframes[0]
    n_rows = int(sum(len(d) for d in ds))
    prep = engine.prepare(plan, xs, ds)

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    # Default (`--feed fresh`): what the reference's inference() call covers per batch (tts.py:665-667) -- the host hand-over of a NEW batch (pack +
    # the H2D pull of ids / lengths / durations as the graph's first node), then the whole pass incl. the integer bookkeeping of the durations, which runs on the device
    # inside the captured graph (engine.BatchRunner: capacities instead of a baked-in batch; ops.row_maps_build).  `--streams` runners keep as
    # many batches in flight.  `--feed replay` = rounds 1-2: one prepared batch (host-built maps, outside the clock) replayed from a hipGraph;
    # --eager launches that pass kernel by kernel.
    host_maps = [engine.build_row_maps([len(x) for x in b[0]], b[1], T_CAP) for b in batches]
    # capacities = the exact maximum over the batches this graph serves, forced durations: the BEST case.  The realistic forms -- the
    # decode driver's calibrated capacities with slack and PREDICTED durations, and the driver itself -- ride on the same line as
    # `value_calibrated_caps` / `value_decode_driver`.
    caps = engine.Caps.for_batches(host_maps, slack_steps=args.cap_slack)
    fresh = args.feed == "fresh" and not args.eager
    eager_out = [None]  # --eager: (mel, per-utterance frames) of the last pass
    if args.eager:
        streams = engine.shared_streams(dev, args.streams) if args.streams > 1 else [torch.cuda.current_stream()]

        def one_pass(i, seed):
            with torch.cuda.stream(streams[i % len(streams)]):
                eager_out[0] = engine.run(plan, prep, ops.DROP_RNG, seed=seed)
            return frames
    elif fresh:
        pass_streams = engine.shared_streams(dev, args.streams)  # one pool per process: every later runner set and the decode driver reuse these queues
        runners = [engine.BatchRunner(plan, args.batch, T_CAP, caps, forced=True, stream=pass_streams[j], seed=77 + 1000 * j) for j in range(args.streams)]

        def one_pass(i, seed):
            r, j = runners[i % len(runners)], i % len(batches)
            r.load(batches[j][0], batches[j][1])
            r.replay()
            return bframes[j]
    else:
        pass_streams = engine.shared_streams(dev, args.streams)
        runners = [engine.GraphRunner(plan, prep, stream=pass_streams[j], seed=77 + 1000 * j) for j in range(args.streams)]

        def one_pass(i, seed):
            runners[i % len(runners)].replay()
            return frames

    for i in range(args.warmup):
        one_pass(i, i)
    counter, done, enq = [0], [0], []

    def region():
        done[0] = 0
        t_e = time.perf_counter()
        for _ in range(args.steps):
            counter[0] += 1
            done[0] += one_pass(counter[0], 1000 + counter[0])
        enq.append(time.perf_counter() - t_e)  # host time to ENQUEUE the region's steps (the GPU is still running them)

    from fcl_taco2_amd import sharding

    # every region is reduced over the ranks (MAX time, SUM frames) before the median is taken, so all ranks report the same region
    agg = []
    for t in timed_regions(region, barrier, max(1, args.regions)):
        agg.append(sharding.aggregate_throughput(t, done[0], dist, dev))
    if fresh:  # every timed pass must have been a valid one: capacities held, frame counts as the host computes them
        for r in runners:
            got = r.frames()
            assert sum(got) in bframes, "bench: a device-driven pass disagrees with the host's frame count"
    rates = sorted(f / t for t, f in agg)
    value = rates[len(rates) // 2] if len(rates) % 2 else 0.5 * (rates[len(rates) // 2 - 1] + rates[len(rates) // 2])
    dts = [a[0] for a in agg]
    dt = median(dts)

    out = {
        "metric": "mel-frames/sec (FCL-taco2-%s forward, batch=%d, 80-mel)" % ("S" if args.model == "student" else "T", args.batch),
        "value": value, "unit": "mel-frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32 (exact fp32 MFMA)" if os.environ.get("FCL_PRECISION", "1") == "0" else
                 "f32 via bf16x3-split MFMA operands, fp32 accumulate (max-abs 8e-6 on mel vs the reference; FCL_PRECISION=0 = exact fp32 MFMA)",
        "data": "synthetic",
        "timing": {"statistic": "median over %d timed regions of exactly %d steps each (barrier + synchronize on both sides; MAX over ranks per region)"
                                % (len(dts), args.steps), "region_ms": [round(1e3 * t, 4) for t in dts], "best_ms_per_step": 1e3 * min(dts) / args.steps,
                   "host_enqueue_ms_per_step": 1e3 * median(enq) / args.steps},
        "config": {"workload": "BASELINE configs[1]: FCL-taco2-%s free-running synthesis, batch=%d/GPU, 60-100 phonemes/utt, forced "
                               "durations clip(Poisson(10),1,50), %s frames / %d phoneme rows per batch, prenet dropout on (device RNG), "
                               "closed-form weights" % ("S" if args.model == "student" else "T", args.batch,
                                                        "/".join(str(f) for f in (bframes if fresh else [frames])), n_rows),
                   "parallelism": "%d independent replicas (utterance-sharded, no collective)" % world,
                   "streams_per_gpu": args.streams,
                   "stream_placement": ("measured: the pass streams sit on %d different compute pipes (ops.stream_apart; DESIGN 5 'compute pipes')"
                                        % sum(1 for s_ in pass_streams if getattr(s_, "fcl_placed", False) or s_ is pass_streams[0])
                                        if (fresh or not args.eager) and args.streams > 1 and any(getattr(s_, "fcl_placed", False) for s_ in pass_streams) else "as created"),
                   "timed_per_step": ("host packing of a NEW batch (%d distinct batches round-robin) into a pinned block + one hipGraph launch: the H2D pull of that "
                                      "block (ids, lengths, durations; fcl_feed_copy), encoder, predictors, device-built row maps (fcl_row_maps_build), decoder loop on device "
                                      "live-row counts, postnet; EXACT capacities, forced durations: %d steps / %d frames, per-step row bounds = the maximum over the fed batches "
                                      "(best case; value_calibrated_caps / value_decode_driver are the calibrated-with-slack, predicted-duration forms)"
                                      % (len(batches), caps.lmax, caps.frames)) if fresh else
                                     ("kernel-by-kernel launches of one prepared batch (host-built maps outside the clock)" if args.eager else
                                      "hipGraph replay of one prepared batch (host-built maps outside the clock)")},
    }

    if args.dump_outputs and rank == 0:
        # what a caller of the timed path receives from its LAST step (pass number counter[0]): the packed mel rows of that batch, utterances back
        # to back, and their frame counts
        last = counter[0]
        if args.eager:
            mel, utt = eager_out[0][0], eager_out[0][1]
            utt = utt.resolve() if isinstance(utt, engine.DeviceFrames) else utt
        elif fresh:
            r = runners[last % len(runners)]
            mel, utt = r.mel, r.frames()
        else:
            r = runners[last % len(runners)]
            mel, utt = r.mel, r.utt_frames
        torch.cuda.synchronize()
        utt = np.asarray([int(n) for n in utt], dtype=np.int64)
        out["dumped"] = dump_outputs(args.dump_outputs, {"mel": mel[: int(utt.sum())].float().cpu().numpy(), "utt_frames": utt})

    if args.full and rank == 0 and world == 1:
        # ---- the same workload the way rounds 1-2 timed it (one prepared batch replayed, host maps outside the clock), and with PREDICTED durations
        # (synthetic duration head, SYN.positive_duration_head: the closed-form head predicts ~0 frames) through the same kind of capacity graph
        if fresh:
            # (on the SAME streams: a second set would share hardware queues with the first, DESIGN.md "5+ streams are slower")
            gr = [engine.GraphRunner(plan, prep, stream=runners[j].stream, seed=5 + j) for j in range(args.streams)]
            for i in range(8):
                gr[i % len(gr)].replay()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for i in range(40):
                gr[i % len(gr)].replay()
            torch.cuda.synchronize()
            out["value_replay_only"] = frames * 40 / (time.perf_counter() - t1)
            del gr
            plan_p = SynthesisPlan(SYN.positive_duration_head(sd_np), hp, dev)
            cal = [engine.run(plan_p, engine.prepare(plan_p, b[0]), ops.DROP_RNG, return_intermediates=True)[2]["maps"] for b in batches]
            pl_cap = max(m.lmax for m in cal) + args.cap_slack
            pb = np.ones(pl_cap, dtype=np.int32)
            for m in cal:
                pb[: m.lmax] = np.maximum(pb[: m.lmax], m.live_rows)
            pcaps = engine.Caps(pl_cap, (max(m.n_frames for m in cal) + 255) // 256 * 256, pb)
            pr = [engine.BatchRunner(plan_p, args.batch, T_CAP, pcaps, forced=False, stream=runners[j].stream, seed=9 + j) for j in range(args.streams)]
            pframes = [m.n_frames for m in cal]

            def ppass(i):
                r, j = pr[i % len(pr)], i % len(batches)
                r.load(batches[j][0])
                r.replay()
                return pframes[j]

            for i in range(8):
                ppass(i)
            torch.cuda.synchronize()
            t1, tot = time.perf_counter(), 0
            for i in range(40):
                tot += ppass(i)
            torch.cuda.synchronize()
            pdt = time.perf_counter() - t1
            for r in pr:
                r.frames()  # raises on a violated capacity
            out["predicted_durations"] = {"value": tot / pdt, "unit": "mel-frames/s", "ms_per_step": 1e3 * pdt / 40, "frames_per_batch": pframes,
                                          "note": "same feed, durations PREDICTED inside the graph (duration predictor -> clamp(round(exp(x) - 1), 0) -> device "
                                                  "row maps); synthetic duration head (log-durations ~ N(2.3, 0.35)) on the closed-form weights"}
            # ---- the same feed the way the decode driver sizes it: the bucket is calibrated on ONE eager batch (its exact maps),
            # every count gets decode._grown_caps' shipped slack (steps x1.5 + 4, frames / live rows x1.3), the graph serves the other batches;
            # durations predicted; a batch beyond the capacities is reported by the device and counted (the driver would re-run it eagerly)
            from fcl_taco2_amd import decode as DEC

            t_bucket = (max(len(x) for b in batches for x in b[0]) + 15) // 16 * 16  # the driver's padded-length bucket
            ccaps = DEC._grown_caps(engine, cal[0], args.batch * t_bucket)
            cr = [engine.BatchRunner(plan_p, args.batch, t_bucket, ccaps, forced=False, stream=runners[j].stream, seed=19 + j) for j in range(args.streams)]

            def cpass(i):
                r, j = cr[i % len(cr)], i % len(batches)
                r.load(batches[j][0])
                r.replay()
                return pframes[j]

            for i in range(8):
                cpass(i)
            torch.cuda.synchronize()
            overflow = 0
            for r in cr:
                try:
                    r.frames()
                except Exception:
                    overflow += 1
            t1, tot = time.perf_counter(), 0
            for i in range(40):
                tot += cpass(i)
            torch.cuda.synchronize()
            cdt = time.perf_counter() - t1
            for r in cr:
                try:
                    r.frames()
                except Exception:
                    overflow += 1
            out["value_calibrated_caps"] = tot / cdt if overflow == 0 else None
            out["calibrated_caps"] = {"value": tot / cdt, "unit": "mel-frames/s", "ms_per_step": 1e3 * cdt / 40, "frames_per_batch": pframes,
                                      "overflowed_runners": overflow, "caps": {"steps": ccaps.lmax, "frames": ccaps.frames, "t_bucket": t_bucket},
                                      "exact": {"steps": max(m.lmax for m in cal), "frames": max(m.n_frames for m in cal)},
                                      "note": "fresh feed, PREDICTED durations, capacities = decode._grown_caps(the first batch's exact maps): the shipped slack of "
                                              "the decode driver (steps x1.5 + 4, frames and live rows x1.3 + 32), padded-length bucket of 16"}
            del cr, pr, plan_p
            # ---- the decode driver itself (python -m fcl_taco2_amd.decode): length-sorted manifest, buckets of 16 phonemes, one eager calibration
            # batch per bucket, graphs with slack, D2H of every mel, nothing written; second call = graphs already captured (steady state of a corpus)
            S_, T_ = HP.student_hparams(), HP.teacher_hparams()
            dmodel = SYN.build_model("student", S_, T_, dev).eval()
            dsd = SYN.positive_duration_head(SYN.closed_form_state_dict(HP.param_spec(S_, T_, True)))
            dmodel.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in dsd.items()})
            dmodel = dmodel.to(dev).eval()
            rng_d = np.random.RandomState(0)
            dutts = [("utt%04d" % i, rng_d.randint(1, S_.idim, size=int(rng_d.randint(60, 101))).astype(np.int64)) for i in range(4096)]
            st0, st1 = {}, {}
            f_cold, s_cold = DEC.decode(dmodel, dutts, None, batch_size=args.batch, depth=args.streams, stats=st0)
            f_d, s_d = DEC.decode(dmodel, dutts, None, batch_size=args.batch, depth=args.streams, stats=st1)
            out["value_decode_driver"] = f_d / s_d
            out["decode_driver"] = {"value": f_d / s_d, "unit": "mel-frames/s", "frames": f_d, "seconds": s_d, "device_seconds": st1["device_seconds"],
                                    "first_call": {"value": f_cold / s_cold, "seconds": s_cold, **{k: v for k, v in st0.items() if k != "device_seconds"}},
                                    "stats": {k: v for k, v in st1.items() if k != "device_seconds"},
                                    "note": "fcl_taco2_amd.decode.decode(): 4 096 utterances of 60-100 phonemes, predicted durations, batch %d, %d graphs in flight, "
                                            "synthesis + D2H of every mel into pinned memory, synchronised; first_call includes graph capture and one eager "
                                            "calibration batch per bucket" % (args.batch, args.streams)}
            DEC.release_graphs(dmodel)
            del dmodel

        # ---- live roofline of the dominant kernel: HIP events around every launch; 5 profiled passes, per-kernel MEDIAN over the passes
        # (one pass in ~10 shows a single launch stretched by whatever else the box is doing; a sum would let that outlier pick the "dominant" kernel)
        engine.run(plan, prep, ops.DROP_RNG, seed=99)
        torch.cuda.synchronize()
        passes = []
        for i in range(5):
            _lib.prof_enable(True)
            engine.run(plan, prep, ops.DROP_RNG, seed=i)
            torch.cuda.synchronize()
            passes.append(_lib.prof_collect())
        _lib.prof_enable(False)
        prof = {}
        for k in passes[0]:
            ms = sorted(p_[k]["ms"] for p_ in passes if k in p_)
            ref = passes[0][k]
            prof[k] = {"ms": 3.0 * ms[len(ms) // 2], "launches": 3 * ref["launches"], "flops": 3.0 * ref["flops"], "rows": 3.0 * ref["rows"],
                       "fill_bytes": 3.0 * ref.get("fill_bytes", 0.0)}
        tot_ms = sum(v["ms"] for v in prof.values()) or 1.0
        # the dominant kernel is chosen per kernel FAMILY (template name): the tile-configuration instantiations of one kernel (picked per launch
        # from M, N) are the same code on the same roofline, and splitting them would let a latency-bound helper win by default
        fam = {}
        for k, v in prof.items():
            f = fam.setdefault(k.split("<")[0].split("/")[0], {"ms": 0.0, "launches": 0, "flops": 0.0, "fill_bytes": 0.0, "members": []})
            f["ms"] += v["ms"]
            f["launches"] += v["launches"]
            f["flops"] += v["flops"]
            f["fill_bytes"] += v.get("fill_bytes", 0.0)
            f["members"].append(k)
        dom = max(fam, key=lambda k: fam[k]["ms"])
        d = fam[dom]
        achieved = d["flops"] / (d["ms"] * 1e-3) / 1e12
        # (the exact-fp32 mode has its own PMC pair: rN_pmc_fp32_fetch_size.csv / ..._write_size.csv, collected under FCL_PRECISION=0)
        traffic, traffic_src = pmc_traffic(dom, "fp32" if os.environ.get("FCL_PRECISION", "1") == "0" else "")
        peak, peak_note = mfma_ceiling()
        out["roofline"] = {
            "bound": "mfma", "kernel": dom, "instantiations": sorted(d["members"]), "achieved": achieved, "peak": peak, "unit": "TFLOP/s",
            "frac": achieved / peak, "traffic": traffic, "traffic_source": traffic_src,
            "avg_launch_us": 1e3 * d["ms"] / d["launches"], "launches_per_step": d["launches"] / 3.0,
            "flops_per_launch": d["flops"] / d["launches"], "share_of_kernel_time": d["ms"] / tot_ms,
            "peak_is": peak_note, "achieved_vs_fp32_matrix_peak": achieved / PEAK_F32_MFMA_TFLOPS,
            "note": "achieved = algorithmic fp32-equivalent FLOPs (2*M*N*K of the kernel's launches; no credit for hoisted att_c terms or padded "
                    "rows) / HIP-event duration on the launch stream; peak = the ceiling of the pipe the kernel issues on (frac <= 1 by construction); "
                    "achieved_vs_fp32_matrix_peak (157.3 TFLOP/s, the pipe an exact-fp32 build would use) is informational only.  Durations are of ISOLATED launches "
                    "(eager passes, one at a time, events around every launch): the two-stage 128-row tiles that serve the first decoder steps since round 6 are ~9 % slower "
                    "alone than the 64-row tiles they replaced (frac 0.140 -> 0.127) and 3.4 % faster on `value` -- two of their workgroups share a CU, so the four passes "
                    "in flight interleave better",
        }
        pmc_wl = "fp32" if os.environ.get("FCL_PRECISION", "1") == "0" else ""
        out["roofline"]["binding"] = binding_record(dom, d["ms"], d["fill_bytes"], pmc_wl)
        out["roofline"]["bound_note"] = ("`bound` names the pipe `achieved` / `peak` are quoted on (the contract's field); what LIMITS the loop is `binding`: the per-CU "
                                         "global->LDS delivery rate -- a 64 x 128 tile pulls 24 KB per 32-k chunk for 384 MFMA cycles per SIMD")
        out["kernels"] = {}
        for k, v in sorted(prof.items()):
            e = {"ms_per_step": v["ms"] / 3.0, "launches_per_step": v["launches"] / 3.0, "tflops": v["flops"] / (v["ms"] * 1e-3) / 1e12 if v["ms"] > 0 else 0.0}
            if v.get("fill_bytes"):
                e["mfma_frac"] = e["tflops"] / peak
                b_ = binding_record(k, v["ms"], v["fill_bytes"], pmc_wl)
                if b_:
                    e["binding"] = {kk: b_[kk] for kk in ("achieved_B_per_clk_per_cu", "frac", "lds_idx_active_over_sq_busy")}
            out["kernels"][k] = e

        # ---- CPU baseline: the oracle ("port" of the reference's per-utterance inference) on the host cores
        if not args.no_cpu_baseline:
            from oracle import fcl_oracle as O

            # host cores this process may use (cgroup/affinity aware), capped: the oracle's per-step ops are small and
            # stop scaling (then thrash) well before a 256-thread pool
            try:
                avail = len(os.sched_getaffinity(0))
            except AttributeError:
                avail = os.cpu_count() or 1
            ncores = max(1, min(avail, args.cpu_threads))
            torch.set_num_threads(ncores)
            sd = {k: torch.from_numpy(np.asarray(v)) for k, v in sd_np.items()}
            txs = [torch.from_numpy(x) for x in xs]
            tds = [torch.from_numpy(d_) for d_ in ds]
            done_frames, n_utts, t2 = 0, 0, time.perf_counter()
            with torch.no_grad():
                O.inference(sd, hp, txs[0], dur=tds[0], prenet_keep="rng")  # warm-up
                t2 = time.perf_counter()
                while time.perf_counter() - t2 < args.cpu_seconds:
                    i = n_utts % len(txs)
                    done_frames += int(O.inference(sd, hp, txs[i], dur=tds[i], prenet_keep="rng")["after"].shape[0])
                    n_utts += 1
            cpu_dt = time.perf_counter() - t2
            out["cpu_baseline"] = {
                "value": done_frames / cpu_dt, "unit": "mel-frames/s", "cores": torch.get_num_threads(), "kind": "port",
                "sample": "%d sequential per-utterance inference() calls of the same batch (%d frames, %.1f s) through oracle/fcl_oracle.py "
                          "(torch %s CPU fp32, prenet dropout on)" % (n_utts, done_frames, cpu_dt, torch.__version__),
            }
    if extras:
        kd = extras.get("kd_step", {})
        out["kd_step_ms"] = kd.get("value")  # north_star's second number: student-KD step time (FCL-taco2-T frozen teacher fwd + S fwd/bwd/Adam, batch 32)
        out["kd_step"] = kd
        fx = extras.get("fp32_exact", {})
        out["value_fp32_exact"] = fx.get("value")  # the headline metric with every contraction on exact fp32 MFMAs (FCL_PRECISION=0)
        out["fp32_exact"] = fx
    if rank == 0:
        emit(out)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
