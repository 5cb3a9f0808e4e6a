"""Data-parallel vocoder training without a GPU: how a global batch is cut across ranks, what train_vocoder refuses, the launcher's dry
run, and vocoder_dp.DataParallel on host tensors over a two-process gloo group -- a three-layer torch.nn generator (5 -> 7 -> 6 -> 3) with one module
that is never called, a two-layer discriminator, buckets of 256 bytes so that the generator's arena has several."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIST_ENV = ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "FCL_DP_FORCE_COLLECTIVE", "FCL_VDP_OVERLAP")


@pytest.fixture(scope="module")
def TV():
    import fcl_taco2_amd  # noqa: F401
    from fcl_taco2_amd import train_vocoder

    return train_vocoder


def test_the_shards_of_a_step_are_its_batch_cut_by_rank(TV):
    lengths = [("u%d" % i, 40 + 7 * i) for i in range(5)]
    sampler = TV.Windows(lengths, 20, 2, 64, 8, 3)
    for step in (1, 2, 7):
        whole, noise = sampler.batch(step), sampler.noise(step)
        assert len(whole) == 8 and noise.shape == (8, 1, 20 * 64)
        for world in (1, 2, 4):
            parts = [TV.shard(whole, r, world) for r in range(world)]
            assert all(len(p) == 8 // world for p in parts)
            owner = {}
            for r, p in enumerate(parts):
                for j, item in enumerate(p):
                    assert (r + j * world) not in owner  # disjoint: every position of the batch has one owner
                    owner[r + j * world] = item
            assert [owner[i] for i in range(8)] == whole  # their union is the batch, in order
            for r in range(world):
                rows = TV.shard(noise, r, world)
                assert rows.shape[0] == 8 // world and np.array_equal(rows, noise[[i for i in range(8) if i % world == r]])
        assert TV.shard(whole, 0, 1) == whole


def _argv(tmp_path, *more):
    return ["--wav-dir", str(tmp_path / "wavs"), "--feature-root", str(tmp_path / "feats"), "--train-list", str(tmp_path / "train.txt"), "--outdir",
            str(tmp_path / "out"), "--verbose", "0"] + list(more)


def test_refusals_by_name(TV, tmp_path, monkeypatch):
    for k in DIST_ENV:
        monkeypatch.delenv(k, raising=False)
    with pytest.raises(ValueError, match=r"--gpus 17 is not supported: 1 to 16 ranks"):
        TV.main(_argv(tmp_path, "--gpus", "17"))
    with pytest.raises(ValueError, match=r"--gpus 17"):
        TV.main(_argv(tmp_path, "--gpus", "17", "--dist-backend", "gloo", "--dry-run-launch"))
    # as one rank of two (the environment torch.distributed.run gives a child): refused before the rendezvous and before any file is read
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "1")
    monkeypatch.setenv("LOCAL_RANK", "1")
    with pytest.raises(ValueError, match=r"batch_size=3 is not a multiple of the 2 ranks"):
        TV.main(_argv(tmp_path, "--gpus", "2", "--batch-size", "3"))
    with pytest.raises(ValueError, match=r"batch_size=16 is not a multiple of the 3 ranks"):
        monkeypatch.setenv("WORLD_SIZE", "3")
        TV.main(_argv(tmp_path, "--generator-type", "HiFiGANGenerator"))
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 1)
    with pytest.raises(ValueError, match=r"--dist-backend nccl: 2 ranks but 1 GPU;"):
        TV.main(_argv(tmp_path, "--gpus", "2", "--batch-size", "4"))
    with pytest.raises(ValueError, match=r"--gpus 4 but WORLD_SIZE=2"):
        TV.main(_argv(tmp_path, "--gpus", "4", "--batch-size", "4"))
    assert not (tmp_path / "out").exists()
    TV.check_ranks(2, "gloo", 1)
    TV.check_ranks(2, "nccl", 2)


def test_dry_run_launch_prints_one_line_from_rank_0():
    env = {k: v for k, v in os.environ.items() if k not in DIST_ENV}
    env["PYTHONPATH"] = os.pathsep.join(p for p in (ROOT, env.get("PYTHONPATH")) if p)
    for n in (2, 1):
        r = subprocess.run([sys.executable, "-m", "fcl_taco2_amd.train_vocoder", "--gpus", str(n), "--dry-run-launch"], capture_output=True, text=True,
                           timeout=600, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout
        out = json.loads(lines[0])
        assert out["dry_run"] is True and out["n_gpus"] == n and out["sum_of_ones"] == float(n)


class _Nets(object):
    """what DataParallel needs of a trainer"""

    def __init__(self, seed):
        torch.manual_seed(seed)
        self.gen = torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.Tanh(), torch.nn.Linear(7, 6), torch.nn.Tanh(), torch.nn.Linear(6, 3))
        self.gen.never_called = torch.nn.Linear(2, 2)
        self.disc = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.Tanh(), torch.nn.Linear(4, 1))


def _loss(nets, x, layers=5):
    return nets.gen[:layers](x).square().mean()


def _local(arena, nets, x, layers=5):
    """this rank's own gradient laid out as the arena is, from autograd.grad (which touches no .grad and fires no hook)"""
    flat = torch.zeros_like(arena.flat)
    grads = torch.autograd.grad(_loss(nets, x, layers), arena.params, allow_unused=True)
    for o, p, g in zip(arena.offsets, arena.params, grads):
        if g is not None:
            flat[o : o + p.numel()] = g.reshape(-1)
    return flat


def _arena_worker(rank, port, q):
    try:
        import datetime

        import torch.distributed as dist

        import fcl_taco2_amd  # noqa: F401
        from fcl_taco2_amd.vocoder_dp import ALIGN, DataParallel

        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=2, timeout=datetime.timedelta(seconds=120))
        nets = _Nets(seed=rank)  # (different initial weights: start-up hands out rank 0's)
        x = torch.randn(4, 5, generator=torch.Generator().manual_seed(10 + rank))
        seen = {}
        for overlap in ("1", "0"):
            os.environ["FCL_VDP_OVERLAP"] = overlap
            dp = DataParallel(nets, bucket_bytes=256)
            dp.same_everywhere("generator", 0)  # (raises unless rank 0's weights are on both)
            dp.same_everywhere("discriminator", 0)
            a = dp.arenas["generator"]
            names = {id(p): k for k, p in nets.gen.named_parameters()}
            assert [names[id(p)] for p in a.params] == list(reversed([k for k, _ in nets.gen.named_parameters()]))
            assert all(o % ALIGN == 0 for o in a.offsets) and len(a.bounds) - 1 >= 3
            assert all((a.bounds[i + 1] - a.bounds[i]) * 4 <= 256 or a.bucket_of.count(i) == 1 for i in range(len(a.bounds) - 1))
            want = []
            for layers in (5, 5 if rank == 0 else 3):  # the second pass: rank 1's loss leaves the last layer out, so its parameters get no gradient there
                mine = _local(a, nets, x, layers)
                both = [torch.empty_like(mine) for _ in range(2)]
                dist.all_gather(both, mine)
                want.append((both[0] + both[1]) * 0.5)
            got = []
            for step, layers in enumerate((5, 5 if rank == 0 else 3)):
                dp.begin("generator")
                assert all(p.grad is not None and p.grad.data_ptr() == a.flat.data_ptr() + 4 * o for o, p in zip(a.offsets, a.params))  # the views survive
                assert not bool(a.flat.any())
                _loss(nets, x, layers).backward()
                launched = a.buckets.collectives
                dp.finish("generator")
                assert a.buckets.collectives == (step + 1) * (len(a.bounds) - 1)  # every bucket, on both ranks, whatever had a gradient
                got.append((a.flat.clone(), launched - step * (len(a.bounds) - 1)))
                pad = torch.ones_like(a.flat, dtype=torch.bool)
                for o, p in zip(a.offsets, a.params):
                    pad[o : o + p.numel()] = False
                assert not bool(a.flat[pad].any())  # the padding stays zero
                assert all(p.grad is None for p in nets.gen.never_called.parameters()) and nets.gen[0].weight.grad is not None
            # in the full pass the hooks launch every bucket up to the first whose parameters are incomplete: never_called's are last in parameters(),
            # first in the arena, so nothing can go before finish(); the assertion is on what was exchanged
            assert all(torch.equal(g, w) for (g, _), w in zip(got, want)), "the arena is not (g0 + g1) * 0.5 bit for bit"
            seen[overlap] = got
            dp.detach()
        assert all(torch.equal(a_[0], b_[0]) for a_, b_ in zip(seen["1"], seen["0"]))  # hook-launched and after-backward exchange: bit-equal arenas
        assert all(n == 0 for _, n in seen["0"])  # FCL_VDP_OVERLAP=0: nothing before backward() has returned

        # hooks do launch during backward when the arena's first parameters get their gradient: the discriminator has no unused module
        os.environ["FCL_VDP_OVERLAP"] = "1"
        dp = DataParallel(nets, bucket_bytes=64)
        d = dp.arenas["discriminator"]
        dp.begin("discriminator")
        nets.disc(torch.randn(2, 3, generator=torch.Generator().manual_seed(20 + rank))).square().mean().backward()
        during = d.buckets.collectives
        dp.finish("discriminator")
        assert during == len(d.bounds) - 1 >= 2 and d.buckets.collectives == during

        terms = dp.mean_terms({"mel_loss": 1.0 + rank, "generator_grad_norm": 0.25 * rank})
        bad = dp.mean_terms({"mel_loss": float("nan") if rank == 1 else 2.0})
        total = dp.sum_float64([1.5 * (rank + 1), rank])
        with torch.no_grad():
            if rank == 1:
                nets.gen[2].bias[1] += 1e-7  # one weight, a few units in its last place
        try:
            dp.same_everywhere("generator", 12)
            caught = None
        except RuntimeError as e:
            caught = str(e)
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok", terms, bad["mel_loss"], total, caught))
    except Exception as e:  # reported to the parent
        import traceback

        q.put((rank, "error", traceback.format_exc() + repr(e)))


def test_the_arena_over_a_two_process_gloo_group():
    import socket

    import torch.multiprocessing as mp

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_arena_worker, args=(r, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = sorted(q.get(timeout=300) for _ in range(2))
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    assert all(r[1] == "ok" for r in res), [r[2] for r in res if r[1] != "ok"]
    assert all(p.exitcode == 0 for p in procs)
    (_, _, t0, b0, s0, c0), (_, _, t1, b1, s1, c1) = res
    assert t0 == t1 == {"generator_grad_norm": 0.125, "mel_loss": 1.5}  # the same floats on both ranks
    assert b0 != b0 and b1 != b1  # a NaN on one rank is a NaN on both
    assert s0 == s1 == [4.5, 1.0]
    for c in (c0, c1):
        assert c is not None and "step 12" in c and "generator of rank 1" in c and "2.bias" in c and "no checkpoint" in c
