"""pow_pool_ancestors, pow_pool_fork_points and pow_pool_chain on the GPU against
their host statement (block.BlockPool.ancestor, .fork_point and .chain, which
tests/test_pool_lift_host.py holds against plain walks).  After every query call
every result is compared with the mirror's, the launches with the plan's
(pow_pool_lift_launches restated here, plus the query's own), and lift_info()
with what the history of the pool implies.  The pools are pool_util's, built
on the CPU with hashlib, so they stop near 2,000 blocks (11 levels): levels 12
to 19 and the chain call at 2^20 lanes are in tests/test_pool_deep_gpu.py."""
import ctypes
import random

import numpy as np
import pytest

from mpi_blockchain_amd._lib import POW_EINVAL, PoolLiftInfo, PowError
from mpi_blockchain_amd.block import POOL_NONE, POOL_ROOT, BlockPool
from mpi_blockchain_amd.miner import GpuMiner, StopBoard

import pool_util as pu
from test_pool_stream_gpu import POISON, compare, feed, last_error

pytestmark = pytest.mark.gpu

ALL_ONES = 0xFFFFFFFF


def rows(n: int) -> int:
    """pow_pool_lift_rows: ceil(log2 n) - 1, at least 0."""
    return max((n - 1).bit_length() - 1, 0) if n else 0


def lift_launches(covered: int, size: int, stale: bool) -> int:
    """pow_pool_lift_launches (csrc/pow_host.cpp)."""
    if stale:
        return rows(size)
    if covered >= size:
        return 0
    m, have = size - covered, rows(covered)
    return ((1 if m <= 256 else have) if have else 0) + rows(size) - have


class Table:
    """What the history of a pool implies for its table: told of every add
    and prune, it states every query call's launches and the info around it."""

    def __init__(self):
        self.covered = self.capacity = 0
        self.stale = True

    def added(self, info):
        self.stale = self.stale or bool(info["reranked"])

    def pruned(self, dropped: bool):
        if dropped:
            self.__init__()

    def before(self, pool):
        """lift_info() between calls, but for what the last query call left in rebuilt and extended."""
        fresh = not self.stale and self.capacity >= pool.info()["capacity"]
        covered = self.covered if fresh else 0
        return {"covered": covered, "rows": rows(covered), "capacity": self.capacity,
                "bytes": 4 * self.capacity * rows(self.capacity)}

    def query(self, pool):
        """(the table's launches of a query call now, lift_info() after it)."""
        info = pool.info()
        size, cap = info["size"], info["capacity"]
        stale = self.stale or self.covered == 0 or cap > self.capacity
        n = lift_launches(self.covered, size, stale)
        after = {"covered": size, "rows": rows(size), "capacity": max(cap, self.capacity), "rebuilt": int(stale),
                 "extended": 0 if stale else size - self.covered,
                 "bytes": 4 * max(cap, self.capacity) * rows(max(cap, self.capacity))}
        self.covered, self.capacity, self.stale = size, after["capacity"], False
        return n, after


def subset(d: dict, keys) -> dict:
    return {k: d[k] for k in keys}


def asked(miner, pool, plan):
    """Behind a query call of at least one query: the stats and the table's info against Table.query's."""
    n, after = plan
    s = miner.stats()
    assert (s["launches"], s["hashes"]) == (n + 1, 0), (s, n)
    assert s["kernel_ms"] > 0
    assert pool.lift_info() == after
    return n


def ask_forks(miner, pool, mirror, table, pairs):
    """pow_pool_fork_points over `pairs` against the mirror's, every one."""
    pairs = list(pairs)
    before = pool.lift_info()
    assert subset(before, ("covered", "rows", "capacity", "bytes")) == table.before(pool)
    plan = table.query(pool)
    at, back_a, back_b = pool.fork_points([a for a, _ in pairs], [b for _, b in pairs])
    n = asked(miner, pool, plan)
    assert at.dtype == back_a.dtype == back_b.dtype == np.uint32 and len(at) == len(back_a) == len(back_b) == len(pairs)
    want = [mirror.fork_point(a, b) for a, b in pairs]
    assert list(zip(at.tolist(), back_a.tolist(), back_b.tolist())) == want
    return n


def ask_ancestors(miner, pool, mirror, table, queries):
    """pow_pool_ancestors over `queries` = (pos, steps) against the mirror's, every one."""
    queries = list(queries)
    before = pool.lift_info()
    assert subset(before, ("covered", "rows", "capacity", "bytes")) == table.before(pool)
    plan = table.query(pool)
    out = pool.ancestors([p for p, _ in queries], [s for _, s in queries])
    n = asked(miner, pool, plan)
    assert out.dtype == np.uint32 and out.tolist() == [mirror.ancestor(p, s) for p, s in queries]
    return n


def ask_chain(miner, pool, mirror, table, tip, max_len=None):
    """pow_pool_chain through the C call with a poisoned array one entry longer than it may write."""
    size = len(mirror)
    room = size if max_len is None else max_len
    touched = min(room, size)
    out = (ctypes.c_uint32 * (touched + 1))(*[POISON] * (touched + 1))
    n_out = ctypes.c_size_t(77)
    want = mirror.chain(tip, max_len)
    plan = table.query(pool) if touched else None
    assert pool.L.pow_pool_chain(pool.handle, tip, room, out, ctypes.byref(n_out)) == 0, last_error(pool.L)
    assert n_out.value == len(want) == min(room, mirror.depth[tip])
    assert list(out)[:touched] == want + [POOL_NONE] * (touched - len(want)) and out[touched] == POISON
    s = miner.stats()
    if touched:
        assert (s["launches"], s["hashes"]) == (plan[0] + 1, 0) and pool.lift_info() == plan[1]
    else:
        assert (s["launches"], s["hashes"], s["kernel_ms"]) == (0, 0, 0)
    assert pool.chain(tip, max_len).tolist() == want  # the wrapper, the table up to date
    if touched:
        assert miner.stats()["launches"] == 1
    return want


def every_query(mirror, extra=2):
    n = len(mirror)
    pairs = [(a, b) for a in range(n) for b in range(n)]
    steps = [(p, s) for p in range(n) for s in list(range(mirror.depth[p] + extra + 1)) + [ALL_ONES]]
    return pairs, steps


@pytest.fixture(scope="module")
def miner():
    with GpuMiner(0) as m:
        yield m


@pytest.fixture(scope="module")
def tree():
    return pu.tree(seed=3)


@pytest.fixture(scope="module")
def chain1025():
    return pu.flat_chain(1025, 0, seed=77)


@pytest.fixture(scope="module")
def side(chain1025):
    """A dead branch of 962 blocks on the chain's root, root side first."""
    return pu.mine_chain(chain1025[0], 962, 0, owner=9, created_at=[1_800_000_000 + k for k in range(962)])[::-1]


# ---- the smallest pools: no row, then one ----
def test_smallest_pools(miner, chain1025):
    pool, mirror, table = None, None, Table()
    try:
        for n in (1, 2, 3, 4):
            pool, mirror, infos = feed(miner, [[chain1025[n - 1]]], 0, mirror=mirror, pool=pool)
            table.added(infos[0])
            pairs, steps = every_query(mirror)
            # 1: nothing to make; 2: no row; 3: the first row, over all blocks; 4: one block into it
            assert ask_forks(miner, pool, mirror, table, pairs) == (0, 0, 1, 1)[n - 1]
            assert ask_ancestors(miner, pool, mirror, table, steps) == 0
            assert pool.lift_info()["rows"] == (0, 0, 1, 1)[n - 1]
            for tip in range(n):
                for max_len in (None, 0, 1, n, n + 1):
                    ask_chain(miner, pool, mirror, table, tip, max_len)
        assert mirror.ancestor(3, 3) == 0 and mirror.ancestor(3, 4) == POOL_ROOT
    finally:
        if pool is not None:
            pool.close()


# ---- the tree of 40 ----
@pytest.mark.parametrize("order", ["mined", "shuffled"])
def test_tree(miner, tree, order):
    blocks = list(tree) if order == "mined" else pu.shuffled(tree, 11)[0]
    pool, mirror, infos = feed(miner, [blocks], pu.D)
    with pool:
        table = Table()
        assert pool.lift_info() == {"covered": 0, "rows": 0, "capacity": 0, "rebuilt": 0, "extended": 0, "bytes": 0}
        pairs, steps = every_query(mirror, extra=1)
        assert len(pairs) == 1600
        assert ask_forks(miner, pool, mirror, table, pairs) == rows(40) == 5  # made from nothing
        assert ask_ancestors(miner, pool, mirror, table, steps) == 0          # up to date
        assert pool.lift_info()["bytes"] == 4 * 64 * 5
        for tip in range(40):
            d = mirror.depth[tip]
            for max_len in (0, 1, 5, d, d + 1, None):
                ask_chain(miner, pool, mirror, table, tip, max_len)
        # blocks on the two different roots: no fork point, and the whole of both walks
        roots = [i for i in range(40) if mirror.parent[i] == POOL_ROOT]
        assert len(roots) == 2
        under = {r: [i for i in range(40) if mirror.chain(i)[-1] == r] for r in roots}
        cross = [(a, b) for a in under[roots[0]][:6] for b in under[roots[1]][:6]]
        at, back_a, back_b = pool.fork_points([a for a, _ in cross], [b for _, b in cross])
        assert set(at.tolist()) == {POOL_NONE}
        assert back_a.tolist() == [mirror.depth[a] for a, _ in cross]
        assert back_b.tolist() == [mirror.depth[b] for _, b in cross]
        compare(pool, mirror)  # the queries change none of the pool's answers


# ---- a flat chain of exactly 2^6 blocks, then its 65th ----
def test_flat_chain_of_64_then_65(miner, chain1025):
    pool, mirror, infos = feed(miner, [chain1025[:64]], 0)
    with pool:
        table = Table()
        assert ask_ancestors(miner, pool, mirror, table, [(63, 63), (63, 64), (63, 65), (63, ALL_ONES), (63, 0)]) == 5
        assert pool.ancestors([63, 63, 63], [63, 64, ALL_ONES]).tolist() == [0, POOL_ROOT, POOL_ROOT]
        pairs, steps = every_query(mirror)
        ask_forks(miner, pool, mirror, table, pairs)
        ask_ancestors(miner, pool, mirror, table, steps)
        assert ask_chain(miner, pool, mirror, table, 63) == list(range(63, -1, -1))
        _, _, infos = feed(miner, [[chain1025[64]]], 0, mirror=mirror, pool=pool)
        table.added(infos[0])
        assert infos[0]["capacity"] == 128
        before = pool.lift_info()
        assert (before["covered"], before["capacity"]) == (0, 64)  # the pool has outgrown it: stale
        assert ask_forks(miner, pool, mirror, table, [(64, 0), (0, 64), (64, 63)]) == rows(65) == 6
        info = pool.lift_info()
        assert (info["rebuilt"], info["capacity"], info["bytes"]) == (1, 128, 4 * 128 * 6)
        pairs, steps = every_query(mirror)
        ask_ancestors(miner, pool, mirror, table, steps)
        ask_forks(miner, pool, mirror, table, pairs)
    # the same at a capacity that holds both: the 65th block goes into five rows and adds a sixth over all blocks
    pool, mirror, infos = feed(miner, [chain1025[:64]], 0, reserve=128)
    with pool:
        table = Table()
        assert ask_forks(miner, pool, mirror, table, [(63, 0)]) == 5
        _, _, infos = feed(miner, [[chain1025[64]]], 0, mirror=mirror, pool=pool)
        table.added(infos[0])
        assert ask_ancestors(miner, pool, mirror, table, [(64, 64), (64, 65), (64, 63)]) == 2  # 3 launches in all
        info = pool.lift_info()
        assert (info["rebuilt"], info["extended"], info["rows"], info["covered"]) == (0, 1, 6, 65)
        pairs, steps = every_query(mirror)
        ask_ancestors(miner, pool, mirror, table, steps)
        ask_forks(miner, pool, mirror, table, pairs)


# ---- the chain of 1,025 and the dead side branch of 962 on its root ----
def test_long_chain_and_its_dead_branch(miner, chain1025, side):
    blocks = chain1025 + side
    pool, mirror, infos = feed(miner, [blocks], 0, reserve=len(blocks))
    with pool:
        table = Table()
        tip, dead = 1024, len(blocks) - 1
        assert ask_forks(miner, pool, mirror, table, [(tip, dead), (dead, tip)]) == rows(1987) == 10
        at, back_a, back_b = pool.fork_points([tip], [dead])
        assert (at.tolist(), back_a.tolist(), back_b.tolist()) == ([0], [1024], [962])
        assert ask_chain(miner, pool, mirror, table, tip) == list(range(1024, -1, -1))
        assert ask_chain(miner, pool, mirror, table, dead) == list(range(dead, 1024, -1)) + [0]
        assert ask_chain(miner, pool, mirror, table, tip, 100) == list(range(1024, 924, -1))
        rng = random.Random(4)
        ask_forks(miner, pool, mirror, table, [(rng.randrange(1987), rng.randrange(1987)) for _ in range(1000)])
        ask_ancestors(miner, pool, mirror, table,
                      [(tip, s) for s in (0, 1, 511, 512, 513, 1023, 1024, 1025, 1026, ALL_ONES)] +
                      [(dead, s) for s in (961, 962, 963, 964)] +
                      [(p, rng.randrange(mirror.depth[p] + 2)) for p in rng.sample(range(1987), 500)])


# ---- fed one block at a time, a query after every add ----
def test_a_query_after_every_add(miner, tree):
    blocks, _ = pu.shuffled(tree, 5)
    pool, mirror, table = None, None, Table()
    reranks = 0
    try:
        for k, b in enumerate(blocks, 1):
            pool, mirror, infos = feed(miner, [[b]], pu.D, mirror=mirror, pool=pool)
            table.added(infos[0])
            rng = random.Random(k)
            n = ask_forks(miner, pool, mirror, table, [(k - 1, rng.randrange(k)) for _ in range(8)] + [(k - 1, k - 1)])
            info = pool.lift_info()
            if infos[0]["reranked"]:  # an old block's walk has changed: made from nothing
                reranks += 1
                assert (info["rebuilt"], info["extended"], n) == (1, 0, rows(k))
            elif k > 1:
                passed = rows(k) - rows(k - 1)  # the size has just passed a power of two: a new row over all blocks
                assert (info["rebuilt"], info["extended"]) == (0, 1)
                assert n == (1 if rows(k - 1) else 0) + passed and n <= 2
            pairs, steps = every_query(mirror, extra=1)
            ask_ancestors(miner, pool, mirror, table, steps)
            if k % 8 == 0 or k == 40:
                ask_forks(miner, pool, mirror, table, pairs)
        assert reranks >= 3  # the shuffle brings parents after their children
    finally:
        if pool is not None:
            pool.close()


# ---- the one-workgroup seam ----
def test_adds_of_256_and_257_blocks(miner, chain1025):
    """Runs of linked blocks shuffled inside their batch: at every level a
    lane needs the entry another lane of its launch has just made."""
    pool, mirror, infos = feed(miner, [chain1025[:300]], 0, reserve=1024)
    with pool:
        table = Table()
        rng = random.Random(8)

        def sample(n):
            return [(rng.randrange(n), rng.randrange(n)) for _ in range(1500)] + [(n - 1, 0), (0, n - 1)]

        assert ask_forks(miner, pool, mirror, table, sample(300)) == rows(300) == 8
        _, _, infos = feed(miner, [pu.shuffled(chain1025[300:556], 21)[0]], 0, mirror=mirror, pool=pool)
        table.added(infos[0])
        assert infos[0]["reranked"] == 0
        # 256 new blocks: one workgroup over the eight rows, then the ninth row over all 556 blocks
        assert ask_forks(miner, pool, mirror, table, sample(556)) == 1 + 1
        assert subset(pool.lift_info(), ("rebuilt", "extended", "rows")) == {"rebuilt": 0, "extended": 256, "rows": 9}
        ask_ancestors(miner, pool, mirror, table, [(p, s) for p in range(300, 556) for s in (1, 2, 255, 256, mirror.depth[p])])
        _, _, infos = feed(miner, [pu.shuffled(chain1025[556:813], 22)[0]], 0, mirror=mirror, pool=pool)
        table.added(infos[0])
        assert infos[0]["reranked"] == 0
        # 257 new blocks: one launch per row
        assert ask_forks(miner, pool, mirror, table, sample(813)) == 9
        assert subset(pool.lift_info(), ("rebuilt", "extended", "rows")) == {"rebuilt": 0, "extended": 257, "rows": 9}
        ask_ancestors(miner, pool, mirror, table, [(p, s) for p in range(556, 813) for s in (1, 2, 255, 256, mirror.depth[p])])
        tip = mirror.best
        assert mirror.depth[tip] == 813 and len(ask_chain(miner, pool, mirror, table, tip)) == 813
        # a small batch whose size does not pass a power of two: the one workgroup alone
        _, _, infos = feed(miner, [pu.shuffled(chain1025[813:900], 23)[0]], 0, mirror=mirror, pool=pool)
        table.added(infos[0])
        assert ask_forks(miner, pool, mirror, table, sample(900)) == 1


def test_an_add_of_300_blocks_across_a_row_boundary(miner, chain1025):
    """Both halves of the table's update in one query call: more new blocks
    than the one workgroup takes (300 > 256), so K13a runs per old row over
    them, and a size that passes a power of two (300 -> 600: 8 rows, then 9),
    so the new row runs over all blocks behind them."""
    pool, mirror, infos = feed(miner, [chain1025[:300]], 0, reserve=1024)
    with pool:
        table = Table()
        rng = random.Random(9)

        def sample(n):
            return [(rng.randrange(n), rng.randrange(n)) for _ in range(300)] + [(n - 1, 0), (0, n - 1), (n - 1, 299)]

        assert ask_forks(miner, pool, mirror, table, sample(300)) == rows(300) == 8
        _, _, infos = feed(miner, [pu.shuffled(chain1025[300:600], 24)[0]], 0, mirror=mirror, pool=pool)
        table.added(infos[0])
        assert infos[0]["reranked"] == 0
        assert ask_forks(miner, pool, mirror, table, sample(600)) == 8 + 1 == lift_launches(300, 600, False)
        assert subset(pool.lift_info(), ("rebuilt", "extended", "rows")) == {"rebuilt": 0, "extended": 300, "rows": 9}
        # the ninth row's entries (512 steps) and the old rows' over the new blocks
        ask_ancestors(miner, pool, mirror, table, [(p, s) for p in range(300, 600, 3) for s in (1, 255, 256, 511, 512, mirror.depth[p])])
        tip = mirror.best
        assert mirror.depth[tip] == 600 and len(ask_chain(miner, pool, mirror, table, tip)) == 600


# ---- capacity ----
def test_the_table_follows_the_capacity(miner, tree, chain1025):
    pool, mirror, infos = feed(miner, [tree], pu.D)
    with pool:
        table = Table()
        assert infos[0]["capacity"] == 64 and pool.lift_info()["bytes"] == 0
        pairs, steps = every_query(mirror, extra=1)
        ask_forks(miner, pool, mirror, table, pairs)
        assert subset(pool.lift_info(), ("capacity", "bytes")) == {"capacity": 64, "bytes": 4 * 64 * 5}
        _, _, infos = feed(miner, [chain1025[:50], chain1025[50:90]], pu.D, mirror=mirror, pool=pool)
        for info in infos:
            table.added(info)
        assert len(mirror) == 130 and infos[-1]["capacity"] == 256
        assert subset(pool.lift_info(), ("covered", "capacity")) == {"covered": 0, "capacity": 64}
        rng = random.Random(6)
        assert ask_forks(miner, pool, mirror, table, [(rng.randrange(130), rng.randrange(130)) for _ in range(2000)]) == 7
        assert subset(pool.lift_info(), ("capacity", "bytes", "rebuilt")) == {"capacity": 256, "bytes": 4 * 256 * 7,
                                                                             "rebuilt": 1}
        ask_ancestors(miner, pool, mirror, table, every_query(mirror, extra=1)[1])
    # a pool that is never queried pays nothing
    pool, mirror, _ = feed(miner, [tree], pu.D)
    with pool:
        pool.mark([mirror.best])
        assert pool.lift_info() == {"covered": 0, "rows": 0, "capacity": 0, "rebuilt": 0, "extended": 0, "bytes": 0}


# ---- prune ----
def test_a_prune_frees_the_table(miner, tree):
    pool, mirror, _ = feed(miner, [tree], pu.D)
    with pool:
        table = Table()
        pairs, steps = every_query(mirror, extra=1)
        ask_forks(miner, pool, mirror, table, pairs)
        # a prune that drops nothing leaves the table as it is
        new, info = pool.prune([], 0)
        assert new.tolist() == mirror.prune([], 0) == list(range(40))
        table.pruned(False)
        assert ask_ancestors(miner, pool, mirror, table, steps) == 0
        tip = mirror.best
        new, info = pool.prune([tip])
        want = mirror.prune([tip])
        assert new.tolist() == want and 0 < len(mirror) < 40
        table.pruned(True)
        assert subset(pool.lift_info(), ("covered", "rows", "capacity", "bytes")) == \
            {"covered": 0, "rows": 0, "capacity": 0, "bytes": 0}
        compare(pool, mirror)
        pairs, steps = every_query(mirror, extra=1)
        assert ask_forks(miner, pool, mirror, table, pairs) == rows(len(mirror))
        assert pool.lift_info()["rebuilt"] == 1
        ask_ancestors(miner, pool, mirror, table, steps)
        chains = [ask_chain(miner, pool, mirror, table, i) for i in range(len(mirror))]
        at = pool.fork_points([a for a, _ in pairs], [b for _, b in pairs])
        # a fresh pool fed the survivors answers the same
        survivors = [b for b, j in zip(tree, want) if j != POOL_NONE]
        fresh, fresh_mirror, _ = feed(miner, [survivors], pu.D)
        with fresh:
            again = fresh.fork_points([a for a, _ in pairs], [b for _, b in pairs])
            for x, y in zip(at, again):
                assert x.tobytes() == y.tobytes()
            assert [fresh.chain(i).tolist() for i in range(len(mirror))] == chains
            assert fresh.ancestors([p for p, _ in steps], [s for _, s in steps]).tolist() == \
                pool.ancestors([p for p, _ in steps], [s for _, s in steps]).tolist()
        # the pool goes on: an add, and the table is extended from what the rebuild left
        more = pu.mine_chain(tree[tip], 1, pu.D, owner=3, created_at=[1_700_000_777])
        _, _, infos = feed(miner, [more], pu.D, mirror=mirror, pool=pool)
        table.added(infos[0])
        n = len(mirror)
        assert ask_forks(miner, pool, mirror, table, [(n - 1, b) for b in range(n)]) <= 2
        assert pool.lift_info()["extended"] == 1


# ---- orphans and twins ----
def test_orphans(miner, tree):
    blocks = tree[2:6] + tree[35:39]  # two walks of four blocks whose parents are not there
    pool, mirror, _ = feed(miner, [blocks], pu.D)
    with pool:
        table = Table()
        assert mirror.parent[0] == mirror.parent[4] == POOL_NONE and mirror.depth[3] == mirror.depth[7] == 4
        pairs, steps = every_query(mirror)
        ask_forks(miner, pool, mirror, table, pairs)
        at, back_a, back_b = pool.fork_points([3, 0], [7, 4])
        assert (at.tolist(), back_a.tolist(), back_b.tolist()) == ([POOL_NONE] * 2, [4, 1], [4, 1])
        ask_ancestors(miner, pool, mirror, table, steps)
        assert pool.ancestors([3, 3], [3, 4]).tolist() == [0, POOL_NONE]
        # the parent of the first walk arrives: an adoption, and the table is made again
        _, _, infos = feed(miner, [[tree[1]]], pu.D, mirror=mirror, pool=pool)
        table.added(infos[0])
        assert infos[0]["reranked"] == 1
        pairs, steps = every_query(mirror)
        assert ask_forks(miner, pool, mirror, table, pairs) == rows(9)
        assert pool.lift_info()["rebuilt"] == 1
        ask_ancestors(miner, pool, mirror, table, steps)


def test_twins(miner):
    storm, children = pu.twin_storm(1, 257)
    pool, mirror, _ = feed(miner, [storm], 0)
    with pool:
        table = Table()
        ask_forks(miner, pool, mirror, table, [(c, 3) for c in children] + [(3, c) for c in children])
        at, back_a, back_b = pool.fork_points(children, [3] * len(children))
        assert set(at.tolist()) == {3} and set(back_a.tolist()) == {1} and set(back_b.tolist()) == {0}
        # a block and its twin: their common parent; two twin roots share no block
        at, back_a, back_b = pool.fork_points([children[0], 3], [children[1], 4])
        assert (at.tolist(), back_a.tolist(), back_b.tolist()) == ([3, POOL_NONE], [1, 1], [1, 1])
        rng = random.Random(3)
        ask_forks(miner, pool, mirror, table, [(rng.randrange(804), rng.randrange(804)) for _ in range(2000)])
        ask_ancestors(miner, pool, mirror, table, [(c, s) for c in children for s in (0, 1, 2, 3)])


# ---- ragged launches ----
@pytest.mark.parametrize("k", [1, 64, 65, 256, 257])
def test_ragged_launches(miner, tree, k):
    pool, mirror, _ = feed(miner, [tree], pu.D)
    with pool:
        table = Table()
        rng = random.Random(k)
        ask_forks(miner, pool, mirror, table, [(rng.randrange(40), rng.randrange(40)) for _ in range(k)])
        ask_ancestors(miner, pool, mirror, table, [(rng.randrange(40), rng.randrange(16)) for _ in range(k)])


# ---- the fuzz ----
@pytest.mark.parametrize("seed,difficulty", pu.FUZZ)
def test_fuzz(miner, seed, difficulty):
    blocks = pu.random_pool(seed)
    pool, mirror, _ = feed(miner, [blocks], difficulty)
    with pool:
        table = Table()
        rng = random.Random(seed)
        n = len(mirror)
        assert ask_forks(miner, pool, mirror, table, [(rng.randrange(n), rng.randrange(n)) for _ in range(2000)]) == rows(n)
        queries = []
        for _ in range(2000):
            p = rng.randrange(n)
            d = mirror.depth[p]
            queries.append((p, rng.choice((rng.randrange(d + 3), d - 1, d, d + 1, ALL_ONES))))
        assert ask_ancestors(miner, pool, mirror, table, queries) == 0
        for tip in rng.sample(range(n), 5):
            ask_chain(miner, pool, mirror, table, tip, rng.choice((None, 3, mirror.depth[tip] + 1)))


# ---- the calls' refusals ----
def test_einval_in_the_stated_order_on_a_live_pool(miner, tree):
    """Each case has every LATER fault too, and the message names the first.
    Nothing is written; the pool, the table's info and the context's stats stay."""
    L = miner.L
    pool, mirror, _ = feed(miner, [tree[:5]], pu.D)
    with pool:
        table = Table()
        ask_forks(miner, pool, mirror, table, [(4, 0)])
        stats, lift = miner.stats(), pool.lift_info()
        words = (ctypes.c_uint32 * 5)(*[POISON] * 5)
        n_out = ctypes.c_size_t(77)
        past = (ctypes.c_uint32 * 3)(0, 5, 4)
        fine = (ctypes.c_uint32 * 3)(0, 1, 4)
        never_read = ctypes.cast(ctypes.c_void_p(8), ctypes.POINTER(ctypes.c_uint32))
        many = (1 << 20) + 1
        h = pool.handle
        for k in (1, many, 1 << 40):
            assert L.pow_pool_ancestors(h, None, never_read, k, words) == POW_EINVAL and "null" in last_error(L)
            assert L.pow_pool_ancestors(h, never_read, None, k, words) == POW_EINVAL and "null" in last_error(L)
            assert L.pow_pool_ancestors(h, never_read, never_read, k, None) == POW_EINVAL and "null" in last_error(L)
            assert L.pow_pool_fork_points(h, None, never_read, k, words, words, words) == POW_EINVAL
            assert "null" in last_error(L)
            assert L.pow_pool_fork_points(h, never_read, None, k, words, None, None) == POW_EINVAL and "null" in last_error(L)
            assert L.pow_pool_fork_points(h, never_read, never_read, k, None, words, words) == POW_EINVAL
            assert "null" in last_error(L)
        for k in (many, 1 << 40):
            assert L.pow_pool_ancestors(h, never_read, never_read, k, words) == POW_EINVAL
            assert "too many queries" in last_error(L)
            assert L.pow_pool_fork_points(h, never_read, never_read, k, words, words, words) == POW_EINVAL
            assert "too many queries" in last_error(L)
        assert L.pow_pool_ancestors(h, past, fine, 3, words) == POW_EINVAL
        assert "query 1 names a block past the pool's 5" in last_error(L)
        assert L.pow_pool_fork_points(h, past, fine, 3, words, words, words) == POW_EINVAL and "query 1" in last_error(L)
        assert L.pow_pool_fork_points(h, fine, past, 3, words, words, words) == POW_EINVAL and "query 1" in last_error(L)
        assert L.pow_pool_ancestors(h, fine, past, 3, words) == 0  # a step count is no position
        assert list(words)[:3] == [0, POOL_ROOT, 0] and list(words)[3:] == [POISON] * 2
        words = (ctypes.c_uint32 * 5)(*[POISON] * 5)
        stats, lift = miner.stats(), pool.lift_info()
        assert L.pow_pool_chain(h, 5, 3, None, None) == POW_EINVAL and "null" in last_error(L)
        assert L.pow_pool_chain(h, 5, 3, words, None) == POW_EINVAL and "null" in last_error(L)
        assert L.pow_pool_chain(h, 5, 3, None, ctypes.byref(n_out)) == POW_EINVAL and "null" in last_error(L)
        assert L.pow_pool_chain(h, 5, 1 << 40, None, ctypes.byref(n_out)) == POW_EINVAL and "null" in last_error(L)
        for tip in (5, POOL_NONE, POOL_ROOT):
            assert L.pow_pool_chain(h, tip, 3, words, ctypes.byref(n_out)) == POW_EINVAL
            assert f"tip (block {tip}) past the pool's 5" in last_error(L)
            assert L.pow_pool_chain(h, tip, 0, None, ctypes.byref(n_out)) == POW_EINVAL and "tip" in last_error(L)
        assert L.pow_pool_lift_get_info(h, None) == POW_EINVAL
        assert list(words) == [POISON] * 5 and n_out.value == 77
        assert miner.stats() == stats and pool.lift_info() == lift
        compare(pool, mirror)
        # null backs are allowed, and a null out where nothing is to be written
        assert L.pow_pool_fork_points(h, fine, fine, 3, words, None, None) == 0 and list(words)[:3] == [0, 1, 4]
        assert L.pow_pool_chain(h, 4, 0, None, ctypes.byref(n_out)) == 0 and n_out.value == 0
        assert miner.stats()["launches"] == 0
        _, _, infos = feed(miner, [tree[5:9]], pu.D, mirror=mirror, pool=pool)
        table.added(infos[0])
        ask_forks(miner, pool, mirror, table, every_query(mirror)[0])


def test_no_queries_and_an_empty_pool(miner, tree):
    L = miner.L
    with miner.open_pool(pu.D) as pool:
        nothing = {"covered": 0, "rows": 0, "capacity": 0, "rebuilt": 0, "extended": 0, "bytes": 0}
        n_out = ctypes.c_size_t(77)
        word = (ctypes.c_uint32 * 1)(POISON)
        zero = (ctypes.c_uint32 * 1)(0)
        assert pool.ancestors([], []).tolist() == [] and miner.stats()["launches"] == 0
        assert [x.tolist() for x in pool.fork_points([], [])] == [[], [], []] and miner.stats()["launches"] == 0
        assert L.pow_pool_ancestors(pool.handle, None, None, 0, None) == 0
        assert L.pow_pool_fork_points(pool.handle, None, None, 0, None, None, None) == 0
        assert L.pow_pool_ancestors(pool.handle, zero, zero, 1, word) == POW_EINVAL and "past the pool's 0" in last_error(L)
        assert L.pow_pool_fork_points(pool.handle, zero, zero, 1, word, None, None) == POW_EINVAL
        assert L.pow_pool_chain(pool.handle, 0, 4, word, ctypes.byref(n_out)) == POW_EINVAL
        assert "tip (block 0) past the pool's 0" in last_error(L)
        with pytest.raises(ValueError):
            BlockPool(pu.D).chain(0)
        assert word[0] == POISON and n_out.value == 77 and pool.lift_info() == nothing
        # k == 0 on a pool that holds blocks: no GPU work and no table work
        mirror = BlockPool(pu.D)
        feed(miner, [tree[:9]], pu.D, mirror=mirror, pool=pool)
        assert pool.ancestors([], []).tolist() == [] and miner.stats() == {"kernel_ms": 0, "launches": 0, "hashes": 0}
        assert pool.lift_info() == nothing
        ask_forks(miner, pool, mirror, Table(), every_query(mirror)[0])


def test_a_context_bound_to_a_stop_board_refuses_the_queries(tree):
    with GpuMiner(0) as m, StopBoard(2) as board:
        L = m.L
        pool, mirror, _ = feed(m, [tree[:5]], pu.D)
        with pool:
            m.bind_board(board, 0, 1)
            try:
                words = (ctypes.c_uint32 * 5)(*[POISON] * 5)
                n_out = ctypes.c_size_t(77)
                at = (ctypes.c_uint32 * 1)(4)
                assert L.pow_pool_ancestors(pool.handle, at, at, 1, words) == POW_EINVAL
                assert "pow_pool_ancestors does not run on a context bound to a stop board" in last_error(L)
                assert L.pow_pool_fork_points(pool.handle, at, at, 1, words, words, words) == POW_EINVAL
                assert "pow_pool_fork_points does not run on a context bound to a stop board" in last_error(L)
                assert L.pow_pool_chain(pool.handle, 4, 5, words, ctypes.byref(n_out)) == POW_EINVAL
                assert "pow_pool_chain does not run on a context bound to a stop board" in last_error(L)
                assert list(words) == [POISON] * 5 and n_out.value == 77
                assert pool.lift_info()["bytes"] == 0  # no GPU work: it answers all the same
            finally:
                m.bind_board(None)
            compare(pool, mirror)
            ask_forks(m, pool, mirror, Table(), every_query(mirror)[0])  # unbound: as before


def test_a_closed_pool_is_not_touched(miner, tree):
    pool, mirror, _ = feed(miner, [tree[:5]], pu.D)
    pool.close()
    for call in (lambda: pool.ancestors([0], [0]), lambda: pool.fork_points([0], [0]), lambda: pool.lift_info()):
        with pytest.raises(PowError, match="null"):
            call()
    n_out = ctypes.c_size_t(77)
    word = (ctypes.c_uint32 * 1)(POISON)
    assert miner.L.pow_pool_chain(pool.handle, 0, 1, word, ctypes.byref(n_out)) == POW_EINVAL
    assert "null pool" in last_error(miner.L) and word[0] == POISON and n_out.value == 77
    assert ctypes.sizeof(PoolLiftInfo) == 32
