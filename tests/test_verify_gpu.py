"""pow_verify_chain on the GPU against its host statement
(mpi_blockchain_amd.block.verify_chain).  The chains are built on the CPU with
hashlib at d = 4 (about 16 trials per block), so no input depends on the code
under test; the expected status is always the mirror's."""
import ctypes
import json
import re

import numpy as np
import pytest

from mpi_blockchain_amd._lib import Block, PowStats
from mpi_blockchain_amd.block import V_WORK, field
from mpi_blockchain_amd.miner import GpuMiner

import verify_util as vu

pytestmark = pytest.mark.gpu

D = 4
BIG = vu.HOST_TILE + 2  # 65,538: two host tiles, one halo block across their seam


@pytest.fixture(scope="module")
def miner():
    with GpuMiner(0) as m:
        yield m


@pytest.fixture(scope="module")
def chain200():
    """The reference's MAX_BLOCKS; every slice of a valid chain is a valid chain."""
    c = vu.build_chain(200, D, seed=5)
    return c, vu.mirror(c, D)


@pytest.fixture(scope="module")
def big_chain():
    """65,538 blocks at difficulty 0: no mining needed."""
    c = vu.build_chain(BIG, 0, seed=6)
    return c, vu.mirror(c, 0)


def check(miner, chain, difficulty, want):
    r = miner.verify_chain(chain, difficulty)
    bad = [i for i, s in enumerate(want) if s]
    assert r.status.dtype == np.uint8 and r.status.tolist() == list(want)
    assert r.first_bad == (bad[0] if bad else len(chain))
    assert r.n_bad == len(bad)
    assert r.ok == (not bad)
    return r


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 129, 200])
def test_valid_chain_lengths(miner, chain200, n):
    c, _ = chain200
    sub = vu.copy_chain(c, 0, n)
    want = vu.mirror(sub, D)
    assert not any(want)
    check(miner, sub, D, want)
    assert miner.stats()["hashes"] == n


def positions(n):
    return sorted({p for p in (0, 63, 64, 65, n - 2, n - 1) if 0 <= p < n})


@pytest.mark.parametrize("kind", list(vu.CORRUPTIONS))
@pytest.mark.parametrize("n", [2, 65, 129, 200])
def test_single_corruptions(miner, chain200, n, kind):
    c, base = chain200
    base = base[:n]  # all zero: the slice's last block only loses checks
    for p in positions(n):
        sub = vu.copy_chain(c, 0, n)
        vu.CORRUPTIONS[kind](sub, p)
        want = vu.expected_after(base, sub, [p, p + 1], D)
        if kind == "index_wrap" and p + 1 < n:
            assert not want[p] & 8  # 0 over 0xFFFFFFFF is consecutive
        else:
            assert any(want) or kind == "index_wrap"
        check(miner, sub, D, want)


def test_three_corruptions_at_once(miner, chain200):
    c, base = chain200
    for n in (65, 129, 200):
        sub = vu.copy_chain(c, 0, n)
        vu.flip_nonce(sub, 0)
        vu.break_prev(sub, 63)
        vu.index_off_by_one(sub, n - 1)
        want = vu.mirror(sub, D)
        assert want[0] and want[63] and want[n - 1]
        check(miner, sub, D, want)


def test_mirror_window_equals_full_mirror(chain200):
    """expected_after (used where the full mirror would take a second per
    case) gives the full mirror's answer."""
    c, base = chain200
    sub = vu.copy_chain(c)
    vu.index_wrap(sub, 64)
    assert vu.expected_after(base, sub, [64, 65], D) == vu.mirror(sub, D)


def test_fixture_chain(miner):
    c, d = vu.fixture_chain()
    want = vu.mirror(c, d)
    assert not any(want)
    check(miner, c, d, want)


def test_work_boundary(miner, chain200):
    c, _ = chain200
    z = [vu.leading_zero_bits(b) for b in c]
    zmin = min(z)
    assert zmin >= D
    check(miner, c, zmin, [0] * 200)
    r = check(miner, c, zmin + 1, vu.mirror(c, zmin + 1))
    assert set(r.status.tolist()) == {0, V_WORK} and r.status[z.index(zmin)] == V_WORK
    for d in (33, 256):  # the full-width path: no 4-bit-mined block has 33 zero bits
        check(miner, c, d, [V_WORK] * 200)
    check(miner, c, 0, [0] * 200)


def test_nullable_outputs_and_buffer_reuse(miner, chain200):
    c, _ = chain200
    sub = vu.copy_chain(c)
    vu.flip_hash_digit(sub, 70)
    vu.break_prev(sub, 150)
    want = vu.mirror(sub, D)
    r = check(miner, sub, D, want)
    L = miner.L
    first, bad = ctypes.c_size_t(), ctypes.c_size_t()
    assert L.pow_verify_chain(miner.ctx, sub, 200, D, None, ctypes.byref(first), ctypes.byref(bad)) == 0
    assert (first.value, bad.value) == (r.first_bad, r.n_bad)
    assert L.pow_verify_chain(miner.ctx, sub, 200, D, None, None, None) == 0
    # a smaller chain after a larger one, through the same device buffers
    small = vu.copy_chain(sub, 69, 72)
    check(miner, small, D, vu.mirror(small, D))
    s = PowStats()
    assert L.pow_get_stats(miner.ctx, ctypes.byref(s)) == 0
    assert s.hashes == 3 and s.launches == 1 and s.kernel_ms > 0
    # bad arguments on a live context
    assert L.pow_verify_chain(miner.ctx, sub, 200, 257, None, None, None) == -1
    assert L.pow_verify_chain(miner.ctx, None, 3, D, None, None, None) == -1
    assert L.pow_verify_chain(miner.ctx, None, 0, D, None, ctypes.byref(first), ctypes.byref(bad)) == 1
    assert (first.value, bad.value) == (0, 0)


def test_digests_agree_with_hash_blocks(miner, chain200):
    c, _ = chain200
    sub = vu.copy_chain(c, 0, 130)
    assert miner.verify_chain(sub, D).ok
    stored = [field(b, "block_hash").split(b"\0", 1)[0].decode() for b in sub]
    assert miner.hash_blocks(list(sub)) == stored


def test_host_tile_seam_valid(miner, big_chain):
    c, base = big_chain
    assert not any(base)
    check(miner, c, 0, base)
    st = miner.stats()
    assert st["hashes"] == BIG and st["launches"] == 2


@pytest.mark.parametrize("kind", list(vu.CORRUPTIONS))
def test_host_tile_seam_corruptions(miner, big_chain, kind):
    """One corruption at a time on both sides of the seam (blocks 65,535 and
    65,536) and at the chain's ends, in place and undone afterwards."""
    c, base = big_chain
    T = vu.HOST_TILE
    for p in (T - 1, T, BIG - 2, BIG - 1):
        keep = vu.copy_chain(c, p, min(BIG, p + 2))
        vu.CORRUPTIONS[kind](c, p)
        try:
            check(miner, c, 0, vu.expected_after(base, c, [p, p + 1], 0))
        finally:
            ctypes.memmove(ctypes.byref(c, p * ctypes.sizeof(Block)), keep, ctypes.sizeof(keep))


def test_host_tile_seam_three_at_once(miner, big_chain):
    c, base = big_chain
    T = vu.HOST_TILE
    keep = vu.copy_chain(c, T - 2, T + 2)
    vu.flip_nonce(c, T - 1)
    vu.break_prev(c, T)
    vu.index_off_by_one(c, T - 2)
    try:
        want = vu.expected_after(base, c, [T - 2, T - 1, T], 0)
        assert sum(1 for s in want if s) >= 4
        check(miner, c, 0, want)
    finally:
        ctypes.memmove(ctypes.byref(c, (T - 2) * ctypes.sizeof(Block)), keep, ctypes.sizeof(keep))


def test_network_with_chain_verification(tmp_path):
    """Every rank mines a private branch of 3 blocks, then all migrate: with
    --verify-chain 1 each migration also passes pow_verify_chain."""
    from mpi_blockchain_amd.node import chain_status, run_network

    run = run_network(2, str(tmp_path), difficulty=9, blocks=10,
                      extra_args=("--private-lead", "3", "--verify-chain", "1"))
    assert run.returncode == 0, run.stdout[-2000:]
    assert run.chains
    for r, entries in run.chains.items():
        consistent, _ = chain_status(entries, 10, 9)
        assert consistent, (r, entries)
    assert any(chain_status(e, 10, 9)[1] for e in run.chains.values())
    last = {}
    for m in re.finditer(r"^pow_node verify (\{.*\})$", run.stdout, flags=re.M):
        v = json.loads(m.group(1))
        last[v["rank"]] = v
    assert sorted(last) == [0, 1], run.stdout[-2000:]
    for v in last.values():
        assert v["calls"] >= 1 and v["blocks"] >= v["calls"] and v["ms"] > 0
    assert any(v["rejected"] == 0 for v in last.values())
