"""-m gpu: fcl_feed_copy (csrc/hostio.hip feed_copy_kernel: one workgroup of 1 024 threads pulls a pinned host block into device memory in
eight-byte words) at the sizes where the index arithmetic of such a loop -- the present one, or a chunked one with several loads in flight per
thread -- can go wrong: 16 bytes (two threads), 71 696 bytes (about the bench geometry's block: a multiple of 16, not of 8 192, so the last pass over
the threads is ragged) and 1 MB + 16 (many passes, the last one two threads wide).  A counter pattern fills the block; after the launch the device
copy equals it, guard lines around the copy are intact, the device and host sequence words have advanced by one and the seed word is bumped exactly
when asked.  Two launches back to back see a block repacked in between."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 512  # bytes of 0xFF in front of and behind the device copy
SIZES = (16, 71696, (1 << 20) + 16)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from fcl_taco2_amd import _lib, ops as _ops

    _lib.load()
    return _ops


def pattern(nbytes, salt):
    """a counter pattern: 32-bit word i holds i * 2654435761 + salt (every word of the block differs from its neighbours and between packings)"""
    w = (np.arange(nbytes // 4, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(salt)) & np.uint64(0xFFFFFFFF)
    return w.astype(np.uint32).view(np.uint8)


@pytest.mark.parametrize("nbytes", SIZES)
def test_feed_copy_sizes(ops, nbytes):
    assert nbytes % 16 == 0 and (nbytes == 16 or nbytes % 8192 != 0)
    host = torch.zeros(nbytes, dtype=torch.uint8).pin_memory()
    seq_host = torch.zeros(4, dtype=torch.int32).pin_memory()
    src, seq_host_dev = ops.host_device_ptr(host), ops.host_device_ptr(seq_host)
    full = torch.full((2 * GUARD + nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    dst = full[GUARD: GUARD + nbytes]
    assert dst.data_ptr() % 16 == 0
    dst.zero_()
    seq_dev = torch.full((1,), 40, dtype=torch.int32, device=DEV)
    seed = torch.full((1,), 1000, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()

    def launch(salt, bump):
        host.numpy()[:] = pattern(nbytes, salt)
        ops.feed_copy(dst, src, nbytes, seq_dev, seq_host_dev, seed if bump else None)
        torch.cuda.synchronize()
        assert np.array_equal(dst.cpu().numpy(), pattern(nbytes, salt)), "the device copy differs from the host block"
        assert bool((full[:GUARD] == 0xFF).all()) and bool((full[GUARD + nbytes:] == 0xFF).all()), "a guard line was overwritten"

    launch(1, True)
    assert int(seq_dev.item()) == 41 and int(seq_host[0]) == 41 and int(seed.item()) == 1001
    launch(2, False)  # the block repacked in between: nothing of the first packing may be served again
    assert int(seq_dev.item()) == 42 and int(seq_host[0]) == 42 and int(seed.item()) == 1001
    assert list(seq_host[1:].numpy()) == [0, 0, 0]


def test_two_launches_back_to_back_see_the_repacked_block(ops):
    """No host synchronisation between the launches: the host waits for the first launch's sequence number (as BatchRunner.load does), repacks, and
    the second launch -- already allowed to start -- must read the new packing."""
    nbytes = SIZES[1]
    host = torch.zeros(nbytes, dtype=torch.uint8).pin_memory()
    seq_host = torch.zeros(4, dtype=torch.int32).pin_memory()
    seq_np = seq_host.numpy()
    src, seq_host_dev = ops.host_device_ptr(host), ops.host_device_ptr(seq_host)
    first = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    second = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    seq_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    host.numpy()[:] = pattern(nbytes, 5)
    ops.feed_copy(first, src, nbytes, seq_dev, seq_host_dev)
    spins = 0
    while int(seq_np[0]) != 1:  # the feed's publication: every read of the block has returned
        spins += 1
        assert spins < 20_000_000, "the sequence number never arrived"
    host.numpy()[:] = pattern(nbytes, 6)
    ops.feed_copy(second, src, nbytes, seq_dev, seq_host_dev)
    torch.cuda.synchronize()
    assert np.array_equal(first.cpu().numpy(), pattern(nbytes, 5)) and np.array_equal(second.cpu().numpy(), pattern(nbytes, 6))
    assert int(seq_np[0]) == 2 and int(seq_dev.item()) == 2
