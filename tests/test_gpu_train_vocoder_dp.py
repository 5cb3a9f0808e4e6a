"""Data-parallel vocoder training on the GPU, on the tiny configurations and the synthetic corpus of test_gpu_train_vocoder.py and
test_gpu_train_vocoder_hifigan.py at a global batch of 4.  Ranks are fresh child processes (spawn); a job of two ranks runs once per module and the tests
read what it left; every wait has a time limit, and after a child that failed nothing more is started.  With this process, at most three hold the GPU.

Two ranks share cuda:0 over gloo where the box has one GPU (the exchange is GradBuckets' host-staged one; what is under test is everything around it);
the one-rank RCCL group under FCL_DP_FORCE_COLLECTIVE runs a rank's real schedule with the identity as its collective; RCCL between two GPUs runs where
there are two."""
import hashlib
import json
import os
import queue
import shutil
import socket
import time
import wave

import numpy as np
import pytest
import torch

import test_gpu_train_vocoder as PWG
import test_gpu_train_vocoder_hifigan as HFG
from test_gpu_features import DEV
from test_gpu_train_vocoder import FS, HOP, corpus, states  # noqa: F401  (corpus: the fixture, rebuilt for this module)

pytestmark = pytest.mark.gpu
HFG_TERMS = HFG.TERMS + ("generator_grad_norm", "discriminator_grad_norm")
PWG_TERMS = ("log_stft_magnitude_loss", "adversarial_loss", "real_loss", "fake_loss")  # (not spectral convergence: a ratio of batch norms, per shard)
# Three steps of the same seed at world 2 against world 1 (the one-process driver, untouched by data parallelism): two correct float32 paths.  The ranks
# sum each gradient over half the batch and then average, the one process sums over the whole batch, in another order and in kernels launched on other
# shapes; Adam's and RAdam's first steps turn a last-bit difference of a small gradient into a difference of that weight, so the legs drift apart and no
# bound can be derived.  Measured once on the MI355X, relative to the world-1 leg, two ranks on one GPU over gloo, the worst over steps
# 1 - 3.  HiFi-GAN: 8.64e-06, the generator's gradient norm of step 3 (3.59e-06 at step 2, 2.86e-07 at step 1); the worst loss term is 1.02e-06, the
# discriminator's fake loss of step 2, every other one is below 4e-07 and four are equal to the last bit.  Parallel WaveGAN: 9.73e-04, the adversarial
# term of step 3 (8.03e-04 at step 2; fake loss 7.1e-04, log magnitude 3.9e-05, real loss 5.2e-08).  That one is not rounding: step 1 agrees to 3.7e-08,
# but its spectral-convergence term is a ratio of batch norms that each rank takes over its own half, so from the first update on the two legs follow
# slightly different gradients (§6u, "Semantics"); the term itself is left out of the comparison for that reason.  The margin is 4 x the worst observed
# (§6s's rule).
WORST_SEEN = {"hifigan": 8.64e-06, "pwg": 9.73e-04}
MARGIN = 4
_failed = []  # a child failed or outlived its limit: nothing more is started


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _digest(tr):
    h = hashlib.sha256()
    for net in (tr.gen, tr.disc):
        for k, v in list(net.named_parameters()) + list(net.named_buffers()):
            h.update(k.encode())
            h.update(v.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def _driver_rank(rank, world, port, env, argv, q):
    """one rank of `train_vocoder` under the environment torch.distributed.run would give it"""
    import traceback

    try:
        os.environ.update(env, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
        import fcl_taco2_amd  # noqa: F401
        from fcl_taco2_amd import train_vocoder as TV

        try:
            tr = TV.main(list(argv))
            q.put((rank, "ok", _digest(tr), tr.steps))
        except FloatingPointError as e:
            q.put((rank, "stopped", str(e), None))
    except Exception as e:
        q.put((rank, "error", traceback.format_exc() + repr(e), None))


def _forced_rank(port, runs, q):
    """each of `runs` (plain argv, forced argv) in turn: the one-process driver, then the same under a one-rank RCCL group"""
    import traceback

    try:
        import fcl_taco2_amd  # noqa: F401
        from fcl_taco2_amd import train_vocoder as TV

        seen = []
        for plain, forced in runs:
            for k in ("FCL_DP_FORCE_COLLECTIVE", "RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
                os.environ.pop(k, None)
            tr = TV.main(list(plain))
            assert tr.dp is None
            os.environ.update(FCL_DP_FORCE_COLLECTIVE="1", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_port()))
            tr = TV.main(list(forced))
            b = {net: a.buckets for net, a in tr.dp.arenas.items()}
            seen.append({net: (x.active, x.avg, x.world, x.collectives, len(x.bounds) - 1) for net, x in b.items()})
        q.put((0, "ok", seen, None))
    except Exception as e:
        q.put((0, "error", traceback.format_exc() + repr(e), None))


def _plumbing_rank(rank, port, argv, q):
    """check 1: the real HiFi-GAN trainer's parameters, gradients that are a function of (rank, slot), the four forms of the exchange"""
    import datetime
    import traceback

    try:
        import torch.distributed as dist

        import fcl_taco2_amd  # noqa: F401
        from fcl_taco2_amd import train_vocoder as TV
        from fcl_taco2_amd.vocoder_dp import NETS, DataParallel

        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=2, timeout=datetime.timedelta(seconds=120))
        tr = TV.HiFiGANTrainer(TV.resolve(TV.build_parser().parse_args(argv)), torch.device(DEV))

        def value(r, j, p):
            return torch.sin(torch.arange(p.numel(), device=DEV, dtype=torch.float32) * 0.37 + (j + 1) * (1.0 + 10.0 * r)).view_as(p)

        out = {}
        for direct in ("0", "1"):
            for overlap in ("1", "0"):
                os.environ.update(FCL_DP_GLOO_DIRECT=direct, FCL_VDP_OVERLAP=overlap)
                dp = DataParallel(tr, bucket_bytes=64 << 10)  # (several buckets in either network of the tiny configuration)
                for net in NETS:
                    a = dp.arenas[net]
                    assert a.buckets.active and a.buckets.world == 2 and a.buckets.stage_host == (direct == "0") and len(a.bounds) - 1 >= 2
                    want = torch.zeros_like(a.flat)
                    for j, (o, p) in enumerate(zip(a.offsets, a.params)):
                        want[o : o + p.numel()] = ((value(0, j, p) + value(1, j, p)) * 0.5).view(-1)
                    for _ in range(2):  # (twice: the second pass zeroes and refills memory the first pass's collectives have read)
                        dp.begin(net)
                        views = all(p.grad.data_ptr() == a.flat.data_ptr() + 4 * o for o, p in zip(a.offsets, a.params))
                        # in parameters() order, so that the backward pass meets the parameters in the arena's order
                        sum((p * value(rank, j, p)).sum() for j, p in reversed(list(enumerate(a.params)))).backward()
                        during = a.next
                        dp.finish(net)
                        torch.cuda.synchronize()
                        out[(direct, overlap, net)] = (views, bool(torch.equal(a.flat, want)), during, len(a.bounds) - 1)
                dp.detach()
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok", out, None))
    except Exception as e:
        q.put((rank, "error", traceback.format_exc() + repr(e), None))


def _children(target, argss, limit):
    """start one child per entry of argss (the queue is appended), collect one message from each within `limit` seconds, join them; a child that
    fails, dies or outlives the limit fails the test and stops every later job"""
    import torch.multiprocessing as mp

    if _failed:
        pytest.fail("an earlier child failed (%s): nothing more is started" % _failed[0])
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=tuple(a) + (q,)) for a in argss]
    for p in procs:
        p.start()
    res, deadline = [], time.monotonic() + limit
    while len(res) < len(procs) and time.monotonic() < deadline:
        try:
            res.append(q.get(timeout=1.0))
        except queue.Empty:
            if any(p.exitcode not in (None, 0) for p in procs):
                break
    for p in procs:
        p.join(timeout=max(1.0, min(60.0, deadline - time.monotonic())))
    late = [p for p in procs if p.is_alive()]
    for p in late:
        p.kill()
        p.join(timeout=30)
    codes = [p.exitcode for p in procs]
    if late or len(res) < len(procs) or any(c != 0 for c in codes) or any(r[1] == "error" for r in res):
        _failed.append(getattr(target, "__name__", "child"))
        pytest.fail("children of %s: exit codes %s, %d outlived %d s, messages: %s" % (_failed[-1], codes, len(late), limit,
                                                                                      [r[2] if r[1] == "error" else r[1] for r in res]))
    return sorted(res)


def _argv(mod, corpus, outdir, *more):  # noqa: F811
    """the module's tiny configuration at a global batch of 4, the discriminator from step 2 on, every step logged"""
    argv = mod.argv_of(corpus, outdir, *more)
    for flag, v in (("--batch-size", "4"), ("--discriminator-train-start-steps", "1"), ("--log-interval-steps", "1")):
        argv[argv.index(flag) + 1] = v
    return argv


def _logs(outdir):
    return [r for r in (json.loads(ln) for ln in (outdir / "train_log.jsonl").read_text().splitlines()) if "ms_per_step" in r]


def _world2(mod, corpus, out, backend, *more):  # noqa: F811
    argv = _argv(mod, corpus, out, "--train-max-steps", "3", "--gpus", "2", "--dist-backend", backend, *more)
    port = _port()
    env = {"HSA_ENABLE_IPC_MODE_LEGACY": os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0")}  # (what train_vocoder's own launcher gives its ranks)
    return _children(_driver_rank, [(r, 2, port, env, argv) for r in range(2)], 240)


@pytest.fixture(scope="module")
def TV():
    assert torch.cuda.is_available()
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import train_vocoder

    return train_vocoder


@pytest.fixture(scope="module")
def world1(TV, corpus, tmp_path_factory):  # noqa: F811
    """the one-process legs, 3 steps of each recipe: the parent commit's path"""
    outs = {}
    for name, mod in (("hifigan", HFG), ("pwg", PWG)):
        outs[name] = tmp_path_factory.mktemp("w1_" + name)
        tr = TV.main(_argv(mod, corpus, outs[name], "--train-max-steps", "3"))
        assert tr.dp is None
    return outs


@pytest.fixture(scope="module")
def world2_gloo(corpus, tmp_path_factory):  # noqa: F811
    outs = {}
    for name, mod in (("hifigan", HFG), ("pwg", PWG)):
        outs[name] = tmp_path_factory.mktemp("w2_" + name)
        outs[name + "_ranks"] = _world2(mod, corpus, outs[name], "gloo")
    return outs


def _against_world1(name, terms, one, two):
    a_, b_ = _logs(two), _logs(one)
    assert [r["step"] for r in a_] == [r["step"] for r in b_] == [1, 2, 3]
    worst = {}
    for a, b in zip(a_, b_):
        assert a["generator_lr"] == b["generator_lr"] and a["discriminator_lr"] == b["discriminator_lr"]
        for k in terms:
            assert (a[k] is None) == (b[k] is None), (a["step"], k)
            if a[k] is not None:
                worst[(a["step"], k)] = abs(a[k] - b[k]) / abs(b[k])
    print("%s, world 2 against world 1, relative differences: %s; worst %.3g" % (name, {k: float("%.3g" % v) for k, v in worst.items()}, max(worst.values())))
    assert (3, "adversarial_loss") in worst and (2, "fake_loss") in worst and all(np.isfinite(v) for v in worst.values())
    assert max(worst.values()) <= MARGIN * WORST_SEEN[name], worst


def _checkpoints(TV, corpus, tmp_path, w2, ranks):  # noqa: F811
    from fcl_taco2_amd import vocoder_decode as VD
    from fcl_taco2_amd.kaldi_io import ArkScpWriter

    (_, s0, d0, n0), (_, s1, d1, n1) = ranks
    assert s0 == s1 == "ok" and n0 == n1 == 3 and d0 == d1  # the two ranks' final parameters and buffers: the same bytes
    ck3, _ = states(w2 / "checkpoint-3steps.pkl")
    assert ck3["steps"] == 3 and sorted(p.name for p in w2.glob("checkpoint-*")) == ["checkpoint-2steps.pkl", "checkpoint-3steps.pkl"]
    # two steps at world 2, then two more in one process: the checkpoint does not pin the world size
    out = tmp_path / "resumed"
    shutil.copytree(w2, out)
    tr = TV.main(_argv(HFG, corpus, out, "--resume", str(out / "checkpoint-2steps.pkl"), "--train-max-steps", "4"))
    ck4, flat = states(out / "checkpoint-4steps.pkl")
    assert tr.steps == 4 and ck4["steps"] == 4 and all(bool(torch.isfinite(v).all()) for v in flat.values())
    mel = np.load(corpus / "feats" / "mels" / "u4.npy")
    with ArkScpWriter(str(tmp_path / "feats")) as w:
        w["u4"] = mel
    samples, _ = VD.main(["--checkpoint", str(w2 / "checkpoint-3steps.pkl"), "--feats-scp", str(tmp_path / "feats.scp"), "--outdir", str(tmp_path / "wav"),
                          "--verbose", "0"])
    with wave.open(str(tmp_path / "wav" / "u4_gen.wav")) as f:
        assert f.getframerate() == FS and f.getnframes() == mel.shape[0] * HOP == samples


def test_plumbing_the_arena_is_the_float32_mean_in_every_form_of_the_exchange(corpus, tmp_path):  # noqa: F811
    argv, port = _argv(HFG, corpus, tmp_path), _port()
    r0, r1 = _children(_plumbing_rank, [(r, port, argv) for r in range(2)], 240)
    for _, _, out, _ in (r0, r1):
        assert len(out) == 8
        for (direct, overlap, net), (views, equal, during, buckets) in out.items():
            assert views and equal, (direct, overlap, net)
            assert during == (buckets if overlap == "1" else 0), (direct, overlap, net, during, buckets)  # from the hooks, or after backward()


def test_one_rank_rccl_group_gives_the_checkpoint_of_the_plain_run(corpus, tmp_path):  # noqa: F811
    runs, outs = [], []
    for name, mod in (("hifigan", HFG), ("pwg", PWG)):
        outs.append((tmp_path / (name + "_plain"), tmp_path / (name + "_forced")))
        runs.append(tuple(_argv(mod, corpus, o, "--train-max-steps", "2") for o in outs[-1]))
    ((_, _, seen, _),) = _children(_forced_rank, [(_port(), runs)], 300)
    for per_net in seen:
        for net, (active, avg, world, collectives, buckets) in per_net.items():
            # RCCL's AVG over one rank, issued for every bucket of every backward pass: the generator's in both steps, the discriminator's in step 2
            assert active and avg and world == 1 and collectives == buckets * (2 if net == "generator" else 1), (net, per_net)
    for plain, forced in outs:
        (a_ck, a), (b_ck, b) = states(plain / "checkpoint-2steps.pkl"), states(forced / "checkpoint-2steps.pkl")
        assert a_ck["steps"] == b_ck["steps"] == 2 and set(a) == set(b) and len([k for k in a if k.startswith("optimizer.discriminator")]) > 0
        for k in a:
            assert torch.equal(a[k], b[k]), k
        la, lb = _logs(plain), _logs(forced)
        for ra, rb in zip(la, lb):
            assert {k: v for k, v in ra.items() if k not in ("ms_per_step", "samples_per_second")} == \
                   {k: v for k, v in rb.items() if k not in ("ms_per_step", "samples_per_second")}


def test_world_2_against_world_1_hifigan(world1, world2_gloo):
    _against_world1("hifigan", HFG_TERMS, world1["hifigan"], world2_gloo["hifigan"])
    ev1 = [json.loads(ln) for ln in (world1["hifigan"] / "train_log.jsonl").read_text().splitlines() if "eval_windows" in ln]
    ev2 = [json.loads(ln) for ln in (world2_gloo["hifigan"] / "train_log.jsonl").read_text().splitlines() if "eval_windows" in ln]
    assert [(r["step"], r["eval_windows"], sorted(r)) for r in ev1] == [(r["step"], r["eval_windows"], sorted(r)) for r in ev2] and len(ev2) == 1


def test_world_2_against_world_1_parallel_wavegan(world1, world2_gloo):
    _against_world1("pwg", PWG_TERMS, world1["pwg"], world2_gloo["pwg"])
    (_, s0, d0, _), (_, s1, d1, _) = world2_gloo["pwg_ranks"]
    assert s0 == s1 == "ok" and d0 == d1


def test_checkpoints_of_world_2_resume_in_one_process_and_decode(TV, corpus, world2_gloo, tmp_path):  # noqa: F811
    _checkpoints(TV, corpus, tmp_path, world2_gloo["hifigan"], world2_gloo["hifigan_ranks"])


def test_a_nan_in_one_ranks_mel_stops_both_ranks_at_that_step(TV, corpus, tmp_path):  # noqa: F811
    bad = tmp_path / "feats" / "mels"
    shutil.copytree(corpus / "feats" / "mels", bad)
    m = np.load(bad / "u1.npy")
    m[:, 3] = np.nan
    np.save(bad / "u1.npy", m)
    argv = _argv(HFG, corpus, tmp_path / "out", "--gpus", "2", "--dist-backend", "gloo")
    argv[argv.index("--feature-root") + 1] = str(tmp_path / "feats")
    # step 1 is one pass over the four utterances: u1 is in exactly one rank's half of it
    cfg = TV.resolve(TV.build_parser().parse_args(argv))
    lengths = [(u, np.load(bad / (u + ".npy")).shape[0]) for u in ("u0", "u1", "u2", "u3", "short")]
    sampler = TV.Windows(lengths, cfg["batch_max_steps"] // HOP, 0, HOP, 4, cfg["seed"])
    holders = [r for r in range(2) if any(sampler.utts[k][0] == "u1" for k, _ in TV.shard(sampler.batch(1), r, 2))]
    assert len(holders) == 1
    port = _port()
    res = _children(_driver_rank, [(r, 2, port, {}, argv) for r in range(2)], 240)
    import re

    for _, status, message, _ in res:
        assert status == "stopped" and re.search(r"step 1: (mel_loss|generator_grad_norm) is nan", message), (status, message)
    assert res[0][2] == res[1][2]
    assert not list((tmp_path / "out").glob("checkpoint-*"))


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="RCCL between two ranks needs two GPUs")
def test_real_rccl_at_world_2(TV, corpus, world1, tmp_path):  # noqa: F811
    out = tmp_path / "w2_rccl"
    ranks = _world2(HFG, corpus, out, "nccl")
    _against_world1("hifigan", HFG_TERMS, world1["hifigan"], out)
    _checkpoints(TV, corpus, tmp_path, out, ranks)
