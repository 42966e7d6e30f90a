"""pow_index_blocks on the GPU against its host statement
(mpi_blockchain_amd.block.index_blocks).  The pools are built on the CPU with
hashlib (block.mine_chain and block.mine_race at d = 4 to 8, verify_util's
chains at d = 0), so no input depends on the code under test; every expected
value is the mirror's.  The ranking alone, on trees no pool can hold (a cycle,
a list of 131,075 nodes), goes through the test library's pow_test_pool_rank."""
import ctypes

import numpy as np
import pytest

from mpi_blockchain_amd._lib import Block, PowStats
from mpi_blockchain_amd.block import (POOL_NONE, POOL_ROOT, V_HASH, V_INDEX, V_LINK, V_WORK, chain_from, index_blocks)
from mpi_blockchain_amd.miner import GpuMiner

import pool_util as pu
import verify_util as vu
from pool_util import check  # one call against the mirror: all five results and the stats

pytestmark = pytest.mark.gpu

T = vu.HOST_TILE
SIZE_MAX = ctypes.c_size_t(-1).value


@pytest.fixture(scope="module")
def miner():
    with GpuMiner(0) as m:
        yield m


@pytest.fixture(scope="module")
def tree():
    return pu.tree(seed=3)


@pytest.fixture(scope="module")
def chain65():
    return pu.flat_chain(65, 0, seed=31)


@pytest.mark.parametrize("n", [0, 1, 2, 3, 63, 64, 65])
def test_sizes_around_the_wave_tile(miner, chain65, n):
    pool, perm = pu.shuffled(chain65[:n], 100 + n)  # a chain's first n blocks from its root are a chain
    r = check(miner, pool, 0)
    assert r.ok and (r.best is None) == (n == 0)
    if n:
        assert pool[r.best].index == n and r.depth[r.best] == n and r.n_bad.tolist() == [0] * n
        assert sorted(r.depth.tolist()) == list(range(1, n + 1))


def test_forked_tree_and_its_permutation(miner, tree):
    """The same pool under a random permutation gives the permuted results,
    and *best names the same block."""
    a = check(miner, tree, pu.D)  # mining order: every parent in front of its children
    assert a.ok and a.best is not None and a.depth[a.best] == 17
    pool, perm = pu.shuffled(tree, 7)
    b = check(miner, pool, pu.D)
    where = {p: k for k, p in enumerate(perm)}  # position in `tree` -> position in `pool`
    for k, p in enumerate(perm):
        assert (b.status[k], b.depth[k], b.n_bad[k]) == (a.status[p], a.depth[p], a.n_bad[p])
        assert b.parent[k] == (where[int(a.parent[p])] if a.parent[p] < 40 else a.parent[p])
    assert perm[b.best] == a.best


def test_host_tile_seam(miner):
    """65,537 blocks at d = 0 in a random order: two host tiles, parents on
    both sides of the seam, a list 17 rounds deep; one tampered block in its
    middle flags the half above it."""
    n = T + 1
    c = vu.build_chain(n, 0, seed=8)  # tip first
    vu.flip_hash_digit(c, n // 2)
    rows = np.frombuffer(c, dtype=np.uint8).reshape(n, ctypes.sizeof(Block))
    perm = np.random.default_rng(9).permutation(n)
    pool = (Block * n).from_buffer_copy(np.ascontiguousarray(rows[perm]).tobytes())
    want = index_blocks(pool, 0)
    status, parent, depth, n_bad, best = want
    assert sum(1 for s in status if s) == 2 and status[int(np.where(perm == n // 2)[0][0])] == V_HASH
    assert max(depth) == n - n // 2 and parent.count(POOL_NONE) == 1 and parent.count(POOL_ROOT) == 1
    r = check(miner, pool, 0, want)
    assert miner.stats()["launches"] == 2 + 3 + 17 and not r.ok
    assert perm[r.best] == n // 2 + 1 and r.n_bad[r.best] == 0  # the block under the tampered one


# ---- every flag and every parent rule ----
def test_tampered_text_takes_the_name_away(miner, tree):
    blocks = [pu.copy_block(b) for b in tree]
    vu.flip_hash_digit(blocks, 5)  # the trunk's fifth block: the next trunk block and the branch's first hang on it
    pool, perm = pu.shuffled(blocks, 13)
    r = check(miner, pool, pu.D)
    at = perm.index(5)
    assert r.status[at] == V_HASH and r.parent[at] < 40
    children = [k for k in range(40) if pool[k].previous_block_hash == pu.name_of(tree[5])]
    assert len(children) == 2 and all(r.status[k] == V_LINK and r.parent[k] == POOL_NONE for k in children)
    # a forged block that copies an honest block's stored text does not shadow it, wherever it stands
    forged = pu.copy_block(tree[5])
    vu.flip_nonce([forged], 0)
    for f, pool in ((0, [forged] + list(tree)), (40, list(tree) + [forged])):
        r = check(miner, pool, pu.D)
        assert r.status[f] & V_HASH and r.n_bad.tolist().count(0) == 40  # (its new digest may lack the work too)
        assert not any(s for k, s in enumerate(r.status) if k != f)


def test_diff_bits_above_what_a_block_has(miner, tree):
    z = [vu.leading_zero_bits(b) for b in tree]
    d = min(z[0], z[32])  # both roots still pass
    assert min(z) < d
    r = check(miner, tree, d)
    assert set(r.status.tolist()) == {0, V_WORK} and [s == V_WORK for s in r.status] == [k < d for k in z]
    r = check(miner, tree, 256)
    assert r.best is None and r.status.tolist() == [V_WORK] * 40 and r.n_bad.tolist() == r.depth.tolist()
    assert check(miner, tree, 0).ok


def test_middle_block_removed(miner, chain65):
    pool = chain65[:4] + chain65[5:9]
    r = check(miner, pool, 0)
    assert r.status.tolist() == [0, 0, 0, 0, V_LINK, 0, 0, 0] and r.parent[4] == POOL_NONE
    assert r.depth.tolist() == [1, 2, 3, 4, 1, 2, 3, 4] and r.n_bad.tolist() == [0, 0, 0, 0, 1, 1, 1, 1] and r.best == 3


def test_index_rule(miner):
    c = pu.flat_chain(4, 0, seed=21)
    c[2].index += 1 << 8  # not hashed
    r = check(miner, c, 0)
    assert r.status.tolist() == [0, 0, V_INDEX, V_INDEX] and r.best == 1
    w = vu.build_chain(3, 0, seed=23)  # tip first: index 0 over 0xFFFFFFFF
    vu.index_wrap(w, 0)
    vu.seal(w[1], 0, 5)
    ctypes.memmove(ctypes.addressof(w[0]) + Block.previous_block_hash.offset,
                   ctypes.addressof(w[1]) + Block.block_hash.offset, 256)
    vu.seal(w[0], 0, 5)
    r = check(miner, w, 0)
    assert r.status.tolist() == [0, V_INDEX, 0] and r.parent.tolist() == [1, 2, POOL_ROOT]


def test_duplicates_in_both_orders(miner, chain65):
    c = chain65[:3]
    for pool, par in (([c[0], c[1], pu.copy_block(c[1]), c[2]], 1), ([c[2], pu.copy_block(c[1]), c[0], c[1]], 1),
                      ([c[1], c[2], c[0], pu.copy_block(c[1])], 0)):
        r = check(miner, pool, 0)
        assert r.ok and r.parent[pool.index(c[2])] == par and r.depth.tolist().count(2) == 2
    # equal digests with indices 1 and 257: the child's V_INDEX follows the lower position
    root = pu.genesis(41, 0, index=1)
    twin = pu.copy_block(root)
    twin.index = 257
    child = pu.flat_chain(2, 0, seed=41)[1]
    assert child.index == 2 and child.previous_block_hash == pu.name_of(root)
    r = check(miner, [root, twin, child], 0)
    assert r.status.tolist() == [0, 0, 0] and r.parent.tolist() == [POOL_ROOT, POOL_ROOT, 0] and r.best == 1
    r = check(miner, [twin, root, child], 0)
    assert r.status.tolist() == [0, 0, V_INDEX] and r.parent.tolist() == [POOL_ROOT, POOL_ROOT, 0] and r.best == 0


def _upper(name: bytes) -> bytes:
    at = next(k for k, ch in enumerate(name) if ch in b"abcdef")
    return name[:at] + name[at:at + 1].upper() + name[at + 1:]


PREV_RULES = {  # what the child carries, given its parent's name -> whom it finds
    "bytes_after_the_nul": (lambda name: name + b"\0" + b"z" * 191, "parent"),
    "empty_with_bytes_after_the_nul": (lambda name: b"\0" + name, "root"),
    "uppercase_digit": (_upper, "none"),
    "63_characters": (lambda name: name[:63], "none"),
    "64_and_no_nul": (lambda name: name + b"0", "none"),
    "non_hex_character": (lambda name: name[:20] + b"g" + name[21:], "none"),
    "256_bytes_no_nul": (lambda name: name + b"0" * 192, "none"),
    "another_digest": (lambda name: bytes(reversed(name)), "none"),
}


@pytest.mark.parametrize("rule", sorted(PREV_RULES))
def test_previous_block_hash_rules(miner, chain65, rule):
    make, finds = PREV_RULES[rule]
    root, child = chain65[0], chain65[1]
    odd = pu.with_prev(child, make(pu.name_of(root)))
    r = check(miner, [child, odd, root], 0)  # the plain child beside it
    assert r.parent.tolist() == [2, {"parent": 2, "root": POOL_ROOT, "none": POOL_NONE}[finds], POOL_ROOT]
    assert r.status.tolist() == [0, V_LINK if finds == "none" else 0, 0]  # a root gets neither link nor index flag
    assert r.depth.tolist() == [2, 2 if finds == "parent" else 1, 1]


def test_cross_check_with_verify_chain(miner, tree):
    """For every tip with n_bad == 0, pow_verify_chain on its chain_from chain returns 1."""
    blocks = [pu.copy_block(b) for b in tree]
    vu.flip_nonce(blocks, 15)  # the branch's third block, where the race forks: four orphans and what stands on them
    pool, _ = pu.shuffled(blocks, 17)
    r = check(miner, pool, pu.D)
    sound = [k for k in range(40) if r.n_bad[k] == 0]
    assert 0 < len(sound) < 40
    for k in sound:
        v = miner.verify_chain(chain_from(pool, r.parent.tolist(), k), pu.D)
        assert v.ok and len(v.status) == r.depth[k]
    k = next(k for k in range(40) if r.n_bad[k] == 1 and r.status[k] == 0)
    # a chain on an orphan: its last block gets no link check from pow_verify_chain; n_bad counts the orphan
    chain = chain_from(pool, r.parent.tolist(), k)
    assert miner.verify_chain(chain, pu.D).ok and chain[len(chain) - 1].previous_block_hash != b""


def test_forced_table_size(monkeypatch, tree, chain65):
    """POW_POOL_SLOTS_LOG2 at its minimum (the lowest power of two above n):
    probe runs and the wrap at the table's end, the same results."""
    monkeypatch.setenv("POW_POOL_SLOTS_LOG2", "1")
    with GpuMiner(0, test_hooks=True) as small:
        for pool, d in ((pu.shuffled(chain65[:64], 3)[0], 0), (pu.shuffled(chain65, 4)[0], 0), (pu.shuffled(tree, 5)[0], pu.D),
                        (pu.shuffled(chain65[:63], 6)[0], 0)):  # 63 blocks in 64 slots: one slot stays empty
            check(small, pool, d)
        lost = [b for k, b in enumerate(chain65[:63]) if k != 30]  # a name the full table does not hold
        r = check(small, lost, 0)
        assert r.parent.tolist().count(POOL_NONE) == 1


def test_reuse_on_one_context():
    """300 blocks, then 5, then 300 different ones: the table and the buffers
    are reset and regrown, a stale slot or digest would show."""
    with GpuMiner(0) as m:
        for n, seed in ((300, 51), (5, 52), (300, 53), (2, 54)):
            pool, _ = pu.shuffled(pu.flat_chain(n, 0, seed=seed), seed)
            if n == 300:
                vu.flip_hash_digit(pool, 17)
            r = check(m, pool, 0)
            assert r.ok == (n != 300)


def test_nullable_outputs_and_bad_arguments(miner, tree):
    blocks = [pu.copy_block(b) for b in tree]
    vu.flip_hash_digit(blocks, 9)
    pool, _ = pu.shuffled(blocks, 19)
    full = check(miner, pool, pu.D)
    arr, n, L = pu.as_array(pool), 40, miner.L
    u32p = ctypes.POINTER(ctypes.c_uint32)

    def call(status=False, parent=False, depth=False, bad=False, best=False):
        st = np.full(n, 0xEE, dtype=np.uint8)
        p, d, b = (np.full(n, 0xEEEEEEEE, dtype=np.uint32) for _ in range(3))
        w = ctypes.c_size_t(77)
        rc = L.pow_index_blocks(miner.ctx, arr, n, pu.D, st.ctypes.data_as(ctypes.c_void_p) if status else None,
                                p.ctypes.data_as(u32p) if parent else None, d.ctypes.data_as(u32p) if depth else None,
                                b.ctypes.data_as(u32p) if bad else None, ctypes.byref(w) if best else None)
        assert rc == 0
        for asked, got, want in ((status, st, full.status), (parent, p, full.parent), (depth, d, full.depth),
                                 (bad, b, full.n_bad)):
            assert got.tolist() == (want.tolist() if asked else [0xEE if got.dtype == np.uint8 else 0xEEEEEEEE] * n)
        assert w.value == (full.best if best else 77)

    for alone in range(5):
        call(*[i != alone for i in range(5)])
        call(*[i == alone for i in range(5)])
    call()
    w = ctypes.c_size_t(77)
    assert L.pow_index_blocks(miner.ctx, arr, n, 257, None, None, None, None, ctypes.byref(w)) == -1
    assert L.pow_index_blocks(miner.ctx, arr, (1 << 20) + 1, 0, None, None, None, None, ctypes.byref(w)) == -1
    assert L.pow_index_blocks(miner.ctx, None, n, 0, None, None, None, None, ctypes.byref(w)) == -1
    assert w.value == 77
    assert L.pow_index_blocks(miner.ctx, None, 0, 0, None, None, None, None, ctypes.byref(w)) == 1
    assert w.value == SIZE_MAX
    s = PowStats()
    assert L.pow_get_stats(miner.ctx, ctypes.byref(s)) == 0 and (s.hashes, s.launches, s.kernel_ms) == (0, 0, 0.0)


# ---- the ranking alone ----
@pytest.fixture(scope="module")
def rank():
    with GpuMiner(0, test_hooks=True) as m:
        fn = m.L.pow_test_pool_rank
        fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t,
                       ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
        fn.restype = ctypes.c_int
        u32p = ctypes.POINTER(ctypes.c_uint32)

        def run(nxt):
            nxt = np.ascontiguousarray(nxt, dtype=np.uint32)
            depth, bad = np.full(len(nxt), 0xEEEEEEEE, dtype=np.uint32), np.full(len(nxt), 0xEEEEEEEE, dtype=np.uint32)
            rc = fn(m.ctx, nxt.ctypes.data_as(u32p), len(nxt), depth.ctypes.data_as(u32p), bad.ctypes.data_as(u32p))
            assert rc == 0, m.L.pow_last_error()
            return depth, bad

        yield run


def test_rank_a_long_list(rank):
    """One list of 2^17 + 3 nodes in a random order: 18 rounds, exact depths."""
    n = (1 << 17) + 3
    order = np.random.default_rng(3).permutation(n).astype(np.uint32)  # order[k] is the node at height k + 1
    nxt = np.empty(n, dtype=np.uint32)
    nxt[order[0]] = POOL_ROOT
    nxt[order[1:]] = order[:-1]
    depth, bad = rank(nxt)
    want = np.empty(n, dtype=np.uint32)
    want[order] = np.arange(1, n + 1, dtype=np.uint32)
    assert np.array_equal(depth, want) and not bad.any()


def test_rank_a_cycle_with_a_tail(rank):
    """A 3-cycle with a tail of 4 on it: depth 0 and n_bad all ones on all
    seven; an acyclic list of 5 and an orphan's walk of 2 in the same call are exact."""
    #      cycle 0 -> 1 -> 2 -> 0; tail 6 -> 5 -> 4 -> 3 -> 1; list 11 -> ... -> 7 -> root; 13 -> 12 -> none
    nxt = [1, 2, 0, 1, 3, 4, 5, POOL_ROOT, 7, 8, 9, 10, POOL_NONE, 12]
    depth, bad = rank(nxt)
    assert depth.tolist() == [0] * 7 + [1, 2, 3, 4, 5, 1, 2]
    assert bad.tolist() == [0xFFFFFFFF] * 7 + [0] * 7
    depth, bad = rank([0])  # the smallest cycle, no round at all
    assert depth.tolist() == [0] and bad.tolist() == [0xFFFFFFFF]
    depth, bad = rank([1, 0, 1, POOL_ROOT])
    assert depth.tolist() == [0, 0, 0, 1] and bad.tolist() == [0xFFFFFFFF] * 3 + [0]
