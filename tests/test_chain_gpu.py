"""pow_mine_chain on the GPU against its host statement
(mpi_blockchain_amd.block.mine_chain, hashlib on the CPU): every comparison is
over all 552 bytes of every block.  The statement never runs the code under
test; d <= 12 keeps it at a few thousand hashlib calls per block."""
import ctypes
import os
import random
import subprocess
import threading
import time

import pytest

from mpi_blockchain_amd import _lib
from mpi_blockchain_amd._lib import Block
from mpi_blockchain_amd.block import field, make_block, mine_chain, nonce_from_counter, set_field, verify_chain
from mpi_blockchain_amd.miner import GpuMiner, StopBoard, refresh_template

import chain_util as cu
import helpers

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mpi_blockchain_amd")
SWITCHES = ("POW_CHAIN_BATCH", "POW_CHAIN_FUSED_MAX", "POW_CHAIN_LANES_LOG2")


def miner_with(**switches):
    """A context of the test library whose pow_init saw the given switches."""
    return helpers.hooked_miner(SWITCHES, **switches)


@pytest.fixture(scope="module")
def miner():
    """The shipped library, as built."""
    with GpuMiner(0) as m:
        yield m


@pytest.fixture(scope="module")
def miner_batch4():
    with miner_with(POW_CHAIN_BATCH=4) as m:
        yield m


def times(n, base=1_700_000_000):
    return [base + 13 * k + (k * k) % 7 for k in range(n)]


def check_against_statement(m, parent, n, d, owner, created_at, start, count):
    want = mine_chain(parent, n, d, owner, created_at, start, count)
    assert len(want) == n, "the statement's windows all hold a solution"
    rc, mined, hashes, out = cu.call(m.L, m.ctx, parent, n, d, owner, created_at, start, count)
    assert rc == 1, (rc, m.L.pow_last_error())
    assert mined == n
    assert cu.raw(out) == cu.raw(want)
    s = m.stats()
    assert s["launches"] == n and s["hashes"] == hashes and hashes >= n and s["kernel_ms"] > 0
    return want


# ---- 4: batch boundaries, the race for the lowest counter ----
@pytest.mark.parametrize("d", [0, 1, 6, 11])
def test_nine_blocks_over_two_batch_boundaries(miner_batch4, d):
    want = check_against_statement(miner_batch4, cu.genesis(), 9, d, 2, times(9), 0, 1 << 16)
    if d == 0:  # every counter solves: the lowest is ctr_start itself
        assert all(field(b, "nonce") == nonce_from_counter(0) for b in want)


@pytest.mark.parametrize("n", [1, 2])
def test_first_link_only(miner, n):
    check_against_statement(miner, cu.genesis(), n, 6, 1, times(n), 0, 1 << 16)


@pytest.mark.parametrize("lanes_log2", [0, 7])
def test_result_does_not_depend_on_the_grid(lanes_log2):
    """One workgroup whose lanes walk the window (d = 8 at 2^0 x 256 lanes: most
    blocks need several strides) and as many workgroups as the chip takes."""
    with miner_with(POW_CHAIN_LANES_LOG2=lanes_log2) as m:
        check_against_statement(m, cu.genesis(), 5, 8, 1, times(5), 62 ** 2 - 100, 1 << 14)
        check_against_statement(m, cu.genesis(), 3, 11, 1, times(3), 0, 1 << 16)


def test_nothing_to_mine(miner):
    rc, mined, hashes, out = cu.call(miner.L, miner.ctx, cu.genesis(), 0, 6, 0, None, 0, 1 << 16)
    assert (rc, mined, hashes) == (1, 0, 0)
    assert cu.raw(out) == b"\xA5" * cu.BLOCK_BYTES
    assert miner.stats()["launches"] == 0


def test_clock_is_read_once(miner):
    t0 = int(time.time())
    r = miner.mine_chain(cu.genesis(), 3, 6, 5, None, 0, 1 << 16)
    t1 = int(time.time())
    assert r.complete and r.n_mined == 3
    assert len({b.created_at for b in r.blocks}) == 1 and t0 <= r.blocks[0].created_at <= t1
    assert verify_chain(r.blocks, 6) == [0, 0, 0]


# ---- 5: truncation and layout traps ----
def trap_parent(index):
    rng = random.Random(index)
    p = make_block(index, 77, 3, (1 << 40) + 5, prev=b"p" * 256, nonce=b"nnnnnnnnn")
    set_field(p, "block_hash", bytes(rng.randrange(1, 256) for _ in range(256)))  # no NUL anywhere
    ctypes.memset(ctypes.addressof(p) + 12, 0xEE, 4)   # the padding behind difficulty ...
    ctypes.memset(ctypes.addressof(p) + 546, 0xDD, 6)  # ... and behind block_hash
    return p


@pytest.mark.parametrize("index", [254, 0xFFFFFFFE])
def test_layout_traps(miner_batch4, index):
    created = [(1 << 32) + 1000 + 255 * k for k in range(4)]
    want = check_against_statement(miner_batch4, trap_parent(index), 4, 6, 0x1FF, created, 0, 1 << 16)
    assert [b.index for b in want] == [(index + 4 - i) & 0xFFFFFFFF for i in range(4)]
    # the first block hashes 256 parent bytes without a NUL; the later ones a hex text and the parent's tail
    first, second = want[3], want[2]
    assert b"\0" not in field(first, "previous_block_hash")
    assert field(second, "previous_block_hash")[64] == 0
    assert field(second, "previous_block_hash")[65:] == field(first, "previous_block_hash")[65:]


# ---- 6: counter edges ----
@pytest.mark.parametrize("start", [62 ** 4 - 3, 62 ** 6 - 3, 62 ** 7 - 3, 62 ** 8 - 3, 62 ** 9 - (1 << 12)])
def test_counter_edges(miner, start):
    check_against_statement(miner, cu.genesis(), 3, 4, 0, times(3), start, 1 << 12)


# ---- 7: a window without a solution ----
def test_window_without_a_solution():
    n, d, window = 8, 10, 700
    for base in range(1_700_000_000, 1_700_000_000 + 64 * 1000, 1000):
        want = mine_chain(cu.genesis(), n, d, 4, times(n, base), 0, window)
        if 2 <= len(want) <= 6:
            break
    else:
        pytest.fail("no created_at base stops between blocks 2 and 6")
    k = len(want)
    with miner_with(POW_CHAIN_BATCH=8) as m:
        rc, mined, hashes, out = cu.call(m.L, m.ctx, cu.genesis(), n, d, 4, times(n, base), 0, window)
        assert rc == 0, (rc, m.L.pow_last_error())
        assert mined == k
        assert cu.raw(out[n - k:]) == cu.raw(want)
        assert cu.raw(out[:n - k]) == b"\xA5" * (cu.BLOCK_BYTES * (n - k))
        assert hashes >= window  # the empty window was searched to its end
        assert m.stats()["launches"] == n  # the batch was queued whole; the launches behind the stop did nothing


# ---- 8: fused against the host loop ----
def test_fused_equals_host_loop(miner):
    n, d, window = 6, 14, 1 << 24
    parent, created = cu.genesis(), times(n)
    fused = miner.mine_chain(parent, n, d, 3, created, 0, window)
    assert fused.complete and fused.n_mined == n
    with miner_with(POW_CHAIN_FUSED_MAX=-1) as h:
        loop = h.mine_chain(parent, n, d, 3, created, 0, window)
        assert loop.complete and h.stats()["launches"] >= n
    assert cu.raw(loop.blocks) == cu.raw(fused.blocks)
    with miner_with(POW_CHAIN_FUSED_MAX=32) as f:  # K4 whatever the built threshold is
        forced = f.mine_chain(parent, n, d, 3, created, 0, window)
        assert forced.complete and f.stats()["launches"] == n  # one launch per block
    assert cu.raw(forced.blocks) == cu.raw(fused.blocks)
    last, by_hand = parent, []
    for k in range(n):
        r = miner.mine(refresh_template(last, 3, d, created[k]), 0, window, d)
        assert r is not None
        by_hand.insert(0, r.block)
        last = r.block
    assert cu.raw(by_hand) == cu.raw(fused.blocks)
    assert verify_chain(fused.blocks, d) == [0] * n


# ---- 9: round trip at the reference's MAX_BLOCKS ----
def test_round_trip_200_blocks(miner):
    n, d = 200, 12
    created = times(n)
    r = miner.mine_chain(cu.genesis(), n, d, 6, created, 0, 1 << 20)
    assert r.complete and r.n_mined == n and len(r.blocks) == n
    v = miner.verify_chain(r.blocks, d)
    assert v.ok and v.n_bad == 0
    assert verify_chain(r.blocks, d) == [0] * n
    oldest = r.blocks[n - 1]
    assert oldest.index == 1 and field(oldest, "previous_block_hash") == bytes(256)
    for k in random.Random(9).sample(range(1, n), 3):  # block k of the mining order, re-mined on its parent
        again = mine_chain(r.blocks[n - k], 1, d, 6, [created[k]], 0, 1 << 20)
        assert cu.raw(again) == cu.raw([r.blocks[n - 1 - k]])


# ---- 10: cancel ----
def test_cancel_word_moved_at_entry(miner):
    rc, mined, hashes, out = cu.call(miner.L, miner.ctx, cu.genesis(), 5, 6, 0, times(5), 0, 1 << 16,
                                     cancel=ctypes.byref(ctypes.c_uint32(8)), epoch=7)
    assert (rc, mined, hashes) == (0, 0, 0)
    assert miner.stats()["launches"] == 0
    assert cu.raw(out) == b"\xA5" * (5 * cu.BLOCK_BYTES)


def test_cancel_between_batches():
    n, d = 20000, 10
    with miner_with(POW_CHAIN_BATCH=16) as m:
        m.warmup()
        word = ctypes.c_uint32(0)
        out = (Block * n)()
        mined = ctypes.c_size_t()
        bump = threading.Timer(0.02, lambda: setattr(word, "value", 1))
        bump.start()
        try:
            rc = m.L.pow_mine_chain(m.ctx, ctypes.byref(cu.genesis()), n, d, 0, None, 0, 1 << 20, ctypes.byref(word), 0,
                                    out, ctypes.byref(mined), None)
        finally:
            bump.join()
        assert rc == 0, (rc, m.L.pow_last_error())
        k = mined.value
        assert k < n
        prefix = (Block * k)()
        ctypes.memmove(prefix, ctypes.byref(out, (n - k) * cu.BLOCK_BYTES), k * cu.BLOCK_BYTES)
        assert m.verify_chain(prefix, d).ok
        if k:
            assert prefix[k - 1].index == 1 and prefix[0].index == k


def test_board_bound_context_is_refused():
    with miner_with() as m, StopBoard(2) as board:
        m.bind_board(board, 0, 1)
        try:
            rc, mined, _, _ = cu.call(m.L, m.ctx, cu.genesis(), 2, 6, 0, times(2), 0, 1 << 16)
            assert rc == _lib.POW_EINVAL and mined == 12345
            assert "board" in (m.L.pow_last_error() or b"").decode()
        finally:
            m.bind_board(None)
        check_against_statement(m, cu.genesis(), 2, 6, 0, times(2), 0, 1 << 16)


# ---- 11: the C example ----
def test_c_example(tmp_path):
    exe = str(tmp_path / "mine_chain_fused")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "mine_chain_fused.c"), "-L", PKG, "-lpow_gpu",
                    f"-Wl,-rpath,{PKG}", "-o", exe], check=True)
    p = subprocess.run([exe, "5", "9"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "chain of 5 blocks at difficulty 9: valid" in p.stdout
    assert p.stdout.count("\nblock ") + p.stdout.startswith("block ") == 5
