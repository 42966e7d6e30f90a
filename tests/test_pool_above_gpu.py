"""pow_pool_tips, pow_pool_subtrees and pow_pool_drop on the GPU against their
host statement (block.BlockPool.tips, .subtrees and .drop, which
tests/test_pool_above_host.py holds against the header's definitions in numpy).
After every call every result is compared with the mirror's and the launches
with the header's closed form: 5 for the tips; T + 1 or T + 3 for the subtrees
and T + 3 or T + 6 for a drop, T being the table's launches as the K13 tests
state them (test_pool_lift_gpu.Table).  After every drop the pool is held
against pow_index_blocks on the surviving structs.  The pools are pool_util's,
built on the CPU with hashlib; 2^16 and 2^20 blocks are in
tests/test_pool_above_deep_gpu.py."""
import ctypes
import random

import numpy as np
import pytest

from mpi_blockchain_amd._lib import POW_EINVAL, POW_ENOSPC, PoolInfo, PowError
from mpi_blockchain_amd.block import POOL_NONE, POOL_ROOT, BlockPool, mine_chain, mine_race, prune_structs
from mpi_blockchain_amd.miner import GpuMiner, StopBoard

import pool_above_util as au
import pool_deep_util as du
import pool_util as pu
from test_pool_lift_gpu import Table, ask_ancestors, ask_forks, every_query
from test_pool_prune_gpu import prune_both
from test_pool_stream_gpu import POISON, compare, feed, last_error

pytestmark = pytest.mark.gpu

NOTHING = {"covered": 0, "rows": 0, "capacity": 0, "rebuilt": 0, "extended": 0, "bytes": 0}
FREED = {"covered": 0, "rows": 0, "capacity": 0, "bytes": 0}


def ask_tips(miner, pool, mirror):
    """Both filters, through the C call with a poisoned array one entry longer than the total."""
    for sound_only in (False, True):
        want = mirror.tips(sound_only)
        out = (ctypes.c_uint32 * (len(want) + 1))(*[POISON] * (len(want) + 1))
        n_out = ctypes.c_size_t(77)
        assert pool.L.pow_pool_tips(pool.handle, int(sound_only), out, len(want) + 1, ctypes.byref(n_out)) == 0, last_error(pool.L)
        assert n_out.value == len(want) and list(out) == want + [POISON]
        s = miner.stats()
        if len(mirror):
            assert (s["launches"], s["hashes"]) == (5, 0) and s["kernel_ms"] > 0
        else:  # an empty pool: no GPU work
            assert s == {"kernel_ms": 0, "launches": 0, "hashes": 0}
        got = pool.tips(sound_only)
        assert got.dtype == np.uint32 and got.tolist() == want and pool.n_tips == len(want)
    return mirror.tips()


def ask_subtrees(miner, pool, mirror, table, roots, marks=True):
    """pow_pool_subtrees over `roots` against the mirror's; returns the table's launches of the call."""
    roots = list(roots)
    plan = table.query(pool)
    got = pool.subtrees(roots, marks=marks)
    s = miner.stats()
    assert (s["launches"], s["hashes"]) == (plan[0] + (3 if marks else 1), 0), (s, plan)
    assert s["kernel_ms"] > 0 and pool.lift_info() == plan[1]
    want = mirror.subtrees(roots)
    for g, w in zip(got[:4], want[:4]):
        assert g.dtype == np.uint32 and g.tolist() == w, (roots, g.tolist(), w)
    if marks:
        assert got[4].dtype == np.uint8 and got[4].tolist() == want[4]
    return plan[0]


def do_drop(miner, pool, mirror, table, blocks, roots, difficulty):
    """pow_pool_drop against the mirror's and against pow_index_blocks on the survivors; returns their structs."""
    roots = list(roots)
    n = len(mirror)
    names = [pu.name_of(b) for b in blocks]
    plan = table.query(pool) if roots else None
    want = mirror.drop(roots)
    new, info = pool.drop(roots)
    kept = len(mirror)
    assert new.dtype == np.uint32 and new.tolist() == want and info["size"] == kept
    s = miner.stats()
    if roots:
        assert (s["launches"], s["hashes"]) == (plan[0] + 3 + (3 if 0 < kept < n else 0), 0), (s, plan, kept, n)
    else:  # no roots: the identity, written on the host
        assert s == {"kernel_ms": 0, "launches": 0, "hashes": 0} and want == list(range(n))
    assert (info["adopted"], info["reranked"], info["rehashed"]) == (0, 0, int(kept < n))
    assert info["ok"] == mirror.ok
    table.pruned(kept < n)
    if kept < n:
        assert {k: pool.lift_info()[k] for k in FREED} == FREED  # the table went with the blocks it covered
    compare(pool, mirror)
    survivors = prune_structs(blocks, want)
    assert pool.find(names) == [mirror.find(x) for x in names]
    if survivors:  # byte for byte what pow_index_blocks gives on them
        r, mine = miner.index_blocks(survivors, difficulty), pool.read()
        for a, b in ((r.status, mine.status), (r.parent, mine.parent), (r.depth, mine.depth), (r.n_bad, mine.n_bad)):
            assert a.tobytes() == b.tobytes()
        assert (r.best, r.ok) == (mine.best, mine.ok)
    return survivors


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
def race31():
    """The published shape: a root and 3 rivals over 10 heights, every height's two losers sealed on their own as
    the forks a race leaves.  31 blocks in mining order; (blocks, the winners' positions by height, the losers')."""
    t, d = 1_700_000_000, 4
    g = pu.genesis(17)
    race, winners, _ = mine_race(g, 10, d, owners=(3, 4, 5), created_at=[t + k for k in range(30)])
    race, winners = race[::-1], winners[::-1]
    blocks, won, lost = [g], [], []
    for h in range(10):
        on = g if h == 0 else race[h - 1]
        for r in range(3):
            if r == winners[h]:
                won.append(len(blocks))
                blocks.append(race[h])
            else:
                lost.append(len(blocks))
                blocks += mine_chain(on, 1, d, owner=3 + r, created_at=[t + 3 * h + r])
    assert len(blocks) == 31 and len(won) == 10 and len(lost) == 20
    return blocks, won, lost


@pytest.fixture(scope="module")
def roots600():
    return pu.tie_pool("flagged_maximum_in_the_ragged_wave")[0]


# ---- the smallest pools ----
@pytest.mark.parametrize("n", [1, 2])
def test_smallest_pools(miner, chain1025, n):
    for roots in ([0], [n - 1], [0, n - 1, 0]):
        pool, mirror, _ = feed(miner, [chain1025[:n]], 0)
        with pool:
            table = Table()
            assert ask_tips(miner, pool, mirror) == [n - 1]
            assert ask_subtrees(miner, pool, mirror, table, roots) == 0  # no row to make
            ask_subtrees(miner, pool, mirror, table, range(n), marks=False)
            do_drop(miner, pool, mirror, table, chain1025[:n], roots, 0)
            assert len(mirror) == (0 if 0 in roots else 1)
            assert ask_tips(miner, pool, mirror) == ([] if 0 in roots else [0])


# ---- the wave and workgroup seams: the ballot rank, K12c's partials, K14c's gather ----
@pytest.mark.parametrize("n", [64, 65, 255, 256, 257])
def test_seams(miner, chain1025, roots600, n):
    # every block a tip (one of them flagged): the list is every position, across waves and workgroups
    pool, mirror, _ = feed(miner, [roots600[600 - n:]], 0)
    with pool:
        table = Table()
        assert ask_tips(miner, pool, mirror) == list(range(n)) and len(mirror.tips(True)) == n - 1
        ask_subtrees(miner, pool, mirror, table, [0, n - 1, n // 2])
        do_drop(miner, pool, mirror, table, roots600[600 - n:], [n - 1, 0, 63 % n], 0)
        assert len(mirror) == n - (2 if n == 64 else 3)
    # one chain, shuffled: a subtree of every size, its members anywhere in the launch
    blocks, perm = pu.shuffled(chain1025[:n], n)
    at = {old: new for new, old in enumerate(perm)}
    pool, mirror, _ = feed(miner, [blocks], 0)
    with pool:
        table = Table()
        assert ask_tips(miner, pool, mirror) == [at[n - 1]]
        ask_subtrees(miner, pool, mirror, table, [at[0], at[1], at[n // 2], at[n - 2], at[n - 1], at[63 % n]])
        size, height = pool.subtrees([at[0], at[1], at[n - 1]])[:2]
        assert size.tolist() == [n, n - 1, 1] and height.tolist() == [n - 1, n - 2, 0]
        do_drop(miner, pool, mirror, table, blocks, [at[n // 2]], 0)
        assert len(mirror) == n // 2


# ---- the published 31-block shape: 21 tips, every loser one ----
@pytest.mark.parametrize("order", ["mined", "shuffled"])
def test_published_shape(miner, race31, order):
    mined, won, lost = race31
    blocks, perm = (list(mined), list(range(31))) if order == "mined" else pu.shuffled(mined, 31)
    at = {old: new for new, old in enumerate(perm)}
    won, lost = [at[i] for i in won], [at[i] for i in lost]

    def fed():
        pool, mirror, _ = feed(miner, [blocks], 4)
        return pool, mirror, Table()

    pool, mirror, table = fed()
    with pool:
        last = min([won[-1]] + lost[-2:])  # three tips share the greatest index: the lowest position wins
        assert mirror.ok and mirror.best == last
        tips = ask_tips(miner, pool, mirror)
        assert len(tips) == 21 and tips == sorted(lost + [won[-1]])
        assert ask_subtrees(miner, pool, mirror, table, range(31)) == 4  # the table from nothing: rows(31)
        for r in range(31):                                               # k = 1, up to date: one launch
            assert ask_subtrees(miner, pool, mirror, table, [r], marks=False) == 0
        for a in range(0, 31, 3):                                         # k = 2: nested, apart and equal
            ask_subtrees(miner, pool, mirror, table, [a, (a * 7 + 5) % 31])
        ask_subtrees(miner, pool, mirror, table, list(range(31)) * 2 + [at[0], won[4]])  # k = 64
        size, height, best, best_index = pool.subtrees([at[0]] + won + lost)
        assert size.tolist() == [31] + [28 - 3 * h for h in range(10)] + [1] * 20
        assert height.tolist() == [10] + [9 - h for h in range(10)] + [0] * 20
        assert best.tolist() == [last] * 10 + [won[-1]] + lost and set(best_index.tolist()[:11]) == {mined[0].index + 10}
        do_drop(miner, pool, mirror, table, blocks, [lost[7]], 4)        # a loser: one block goes
        assert len(mirror) == 30 and len(ask_tips(miner, pool, mirror)) == 20
    pool, mirror, table = fed()
    with pool:
        do_drop(miner, pool, mirror, table, blocks, [won[5]], 4)         # a winner: every height above goes with it
        assert len(mirror) == 31 - (1 + 3 * 4)
        tips = ask_tips(miner, pool, mirror)
        assert len(tips) == 2 * 6 and mirror.index[mirror.best] == mined[0].index + 6  # the losers of the six heights left
        ask_subtrees(miner, pool, mirror, table, range(len(mirror)))


def test_a_drop_a_prune_a_drop_and_queries_on_one_pool(miner, race31):
    """The drop and the prune share their second half and nothing else: a
    drop, a plain prune with tips and flags, a second drop and K13 queries on
    one pool, each against the mirror (do_drop, prune_both and ask_ancestors
    hold the launches' closed forms) and against the numpy statements over the
    arrays the pool gave before the call."""
    blocks, won, lost = race31

    def arrays():
        r = pool.read()
        return r.parent, r.depth, np.array(mirror.index, dtype=np.uint32), r.n_bad

    def drop(structs, root):
        parent, depth, index, n_bad = arrays()
        on = au.subtrees_of(parent, depth, index, n_bad, [root])[3]
        _, want_parent, want_depth = au.dropped(parent, depth, 1 - on)
        left = do_drop(miner, pool, mirror, table, structs, [root], 4)
        assert len(left) == len(structs) - int(on.sum()) and miner.stats()["kernel_ms"] > 0
        assert all(a is b for a, b in zip(left, [s for s, gone in zip(structs, on) if not gone]))
        after = pool.read()
        assert after.parent.tolist() == want_parent.tolist() and after.depth.tolist() == want_depth.tolist()
        return left

    pool, mirror, _ = feed(miner, [blocks], 4)
    with pool:
        table = Table()
        structs = drop(list(blocks), lost[7])                       # the table from nothing: rows(31) + 3 + 3 launches
        assert len(structs) == 30
        # a plain prune: one low loser as a tip, and every sound block of the two greatest heights by index
        tip, min_index = mirror.find(pu.name_of(blocks[lost[3]])), blocks[0].index + 9
        parent, depth, index, n_bad = arrays()
        seeds = sorted({tip} | set(np.flatnonzero((index >= min_index) & (n_bad == 0)).tolist()))
        kept, want = du.map_of(du.marks_of(parent, depth, seeds))
        structs, new, info = prune_both(miner, pool, mirror, structs, ([tip], min_index, True))
        assert new == want.tolist() and 0 < kept == len(structs) == info["size"] < 30
        table.pruned(True)
        structs = drop(structs, mirror.find(pu.name_of(blocks[won[8]])))  # the table went with the prune: from nothing
        assert 0 < len(structs) < kept
        _, steps = every_query(mirror)
        ask_ancestors(miner, pool, mirror, table, steps)             # made again behind the drop, then up to date
        parent = pool.read().parent
        for (p, s), got in zip(steps, pool.ancestors([p for p, _ in steps], [s for _, s in steps]).tolist()):
            walk, end = du.plain_walk(parent, p)
            assert got == (walk[s] if s < len(walk) else end), (p, s)
        assert miner.stats()["launches"] == 1 and pool.lift_info()["covered"] == len(structs)


# ---- the tree of 40: two roots, branches of several depths ----
@pytest.mark.parametrize("order", ["mined", "shuffled"])
def test_tree(miner, tree, order):
    blocks = list(tree) if order == "mined" else pu.shuffled(tree, 11)[0]
    pool, mirror, _ = feed(miner, [blocks], pu.D)
    with pool:
        table = Table()
        assert pool.lift_info() == NOTHING
        tips = ask_tips(miner, pool, mirror)
        assert len(tips) == 6 and pool.lift_info() == NOTHING  # the tips need no table
        assert ask_subtrees(miner, pool, mirror, table, range(40)) == 5   # made from nothing: rows(40)
        assert ask_subtrees(miner, pool, mirror, table, [7], marks=False) == 0  # up to date: one launch
        for k in (1, 2, 64):  # duplicates and nested roots
            rng = random.Random(k)
            ask_subtrees(miner, pool, mirror, table, [rng.randrange(40) for _ in range(k)])
        ask_subtrees(miner, pool, mirror, table, [0] * 64)
        both = [i for i in range(40) if mirror.parent[i] == POOL_ROOT]
        size, height, best, best_index, on = pool.subtrees(both, marks=True)
        assert sorted(size.tolist()) == [8, 32] and on.tolist() == [1] * 40
        assert mirror.best in best.tolist()  # the pool's fork choice is one root's
        compare(pool, mirror)  # the queries change none of the pool's answers
        # after a one-block add: the table's one-workgroup launch, then K14d
        more = pu.mine_chain(blocks[tips[0]], 1, pu.D, owner=3, created_at=[1_700_000_777])
        _, _, infos = feed(miner, [more], pu.D, mirror=mirror, pool=pool)
        table.added(infos[0])
        assert ask_subtrees(miner, pool, mirror, table, [tips[0], 40], marks=False) == 1
        assert pool.subtrees([tips[0]])[0].tolist() == [2]


def test_65_roots_are_refused_and_the_order_of_the_checks(miner, tree):
    """Each case has every LATER fault too, and the message names the first.
    Nothing is written; the pool, the table's info and the context's stats stay."""
    L = miner.L
    pool, mirror, _ = feed(miner, [tree[:5]], pu.D)
    with pool:
        table = Table()
        ask_subtrees(miner, pool, mirror, table, [0])
        stats, lift = miner.stats(), pool.lift_info()
        words = (ctypes.c_uint32 * 65)(*[POISON] * 65)
        n_out = ctypes.c_size_t(77)
        info = PoolInfo(*[POISON] * 9)
        past = (ctypes.c_uint32 * 65)(*([0, 5, 4] + [0] * 62))
        h = pool.handle
        for k in (65, 1 << 40):
            assert L.pow_pool_subtrees(h, None, k, words, words, words, words, None, ctypes.byref(n_out)) == POW_EINVAL
            assert "too many roots" in last_error(L)
            assert L.pow_pool_drop(h, None, k, words, ctypes.byref(info)) == POW_EINVAL and "too many roots" in last_error(L)
        assert L.pow_pool_subtrees(h, None, 3, words, None, None, None, None, None) == POW_EINVAL and "null roots" in last_error(L)
        assert L.pow_pool_drop(h, None, 3, words, ctypes.byref(info)) == POW_EINVAL and "null roots" in last_error(L)
        assert L.pow_pool_subtrees(h, past, 3, words, words, words, words, None, ctypes.byref(n_out)) == POW_EINVAL
        assert "root 1 (block 5) past the pool's 5" in last_error(L)
        assert L.pow_pool_drop(h, past, 64, words, ctypes.byref(info)) == POW_EINVAL and "root 1 (block 5)" in last_error(L)
        assert L.pow_pool_tips(h, 2, None, 4, None) == POW_EINVAL and "unknown flags 0x2" in last_error(L)
        assert L.pow_pool_tips(h, 0xFFFFFFFF, words, 4, ctypes.byref(n_out)) == POW_EINVAL and "unknown flags" in last_error(L)
        assert L.pow_pool_tips(h, 1, words, 4, None) == POW_EINVAL and "null" in last_error(L)
        assert L.pow_pool_tips(h, 1, None, 4, ctypes.byref(n_out)) == POW_EINVAL and "null" in last_error(L)
        assert list(words) == [POISON] * 65 and n_out.value == 77 and info.size == POISON
        assert miner.stats() == stats and pool.lift_info() == lift
        compare(pool, mirror)
        # every output of the subtrees may be null, and a null out where nothing is to be written
        assert L.pow_pool_subtrees(h, past, 1, None, None, None, None, None, None) == 0
        assert L.pow_pool_tips(h, 0, None, 0, ctypes.byref(n_out)) == POW_ENOSPC and n_out.value == 1
        ask_subtrees(miner, pool, mirror, table, range(5))


# ---- cap ----
def test_cap(miner, roots600):
    blocks = roots600[:300]
    pool, mirror, _ = feed(miner, [blocks], 0)
    with pool:
        L, total = miner.L, 300
        for cap, rc in ((0, POW_ENOSPC), (1, POW_ENOSPC), (total - 1, POW_ENOSPC), (total, 0), (total + 7, 0)):
            room = max(cap, total) + 9
            out = (ctypes.c_uint32 * room)(*[POISON] * room)
            n_out = ctypes.c_size_t(77)
            assert L.pow_pool_tips(pool.handle, 0, out, cap, ctypes.byref(n_out)) == rc
            assert n_out.value == total
            wrote = min(cap, total)
            assert list(out)[:wrote] == list(range(wrote)) and list(out)[wrote:] == [POISON] * (room - wrote)
            assert rc == 0 or f"{total} tips > cap {cap}" in last_error(L)
            assert miner.stats()["launches"] == 5
        assert pool.tips(cap=10).tolist() == list(range(10)) and pool.n_tips == 300
        assert pool.tips(True, cap=299).tolist() == list(range(299)) and pool.n_tips == 300
        compare(pool, mirror)


# ---- the chain of 1,025: the height reaches 1,024 and the depth differences cross every level ----
def test_chain1025(miner, chain1025):
    blocks, perm = pu.shuffled(chain1025, 4)
    at = {old: new for new, old in enumerate(perm)}
    pool, mirror, _ = feed(miner, [blocks], 0)
    with pool:
        table = Table()
        assert ask_tips(miner, pool, mirror) == [at[1024]]
        cuts = [0, 1, 2, 3, 255, 256, 257, 511, 512, 513, 1022, 1023, 1024]
        assert ask_subtrees(miner, pool, mirror, table, [at[c] for c in cuts]) == 10
        size, height, best, best_index = pool.subtrees([at[c] for c in cuts])
        assert size.tolist() == [1025 - c for c in cuts] and height.tolist() == [1024 - c for c in cuts]
        assert set(best.tolist()) == {at[1024]} and set(best_index.tolist()) == {chain1025[1024].index}
        do_drop(miner, pool, mirror, table, blocks, [at[513]], 0)
        assert len(mirror) == 513 and pool.info()["capacity"] == 1024
        assert ask_tips(miner, pool, mirror) == [mirror.best]


# ---- orphans, twins and POW_V_HASH blocks: tips, roots and members ----
def test_orphans(miner, tree):
    blocks = tree[2:6] + tree[35:39]  # two walks of four blocks whose parents are not there
    pool, mirror, _ = feed(miner, [blocks], pu.D)
    with pool:
        table = Table()
        assert mirror.parent[0] == mirror.parent[4] == POOL_NONE
        assert ask_tips(miner, pool, mirror) == [3, 7] and mirror.tips(True) == []
        ask_subtrees(miner, pool, mirror, table, range(8))
        size, height, best, best_index = pool.subtrees([0, 4, 7])
        assert (size.tolist(), height.tolist(), best.tolist(), best_index.tolist()) == ([4, 4, 1], [3, 3, 0], [POOL_NONE] * 3, [0] * 3)
        do_drop(miner, pool, mirror, table, blocks, [5], pu.D)
        assert len(mirror) == 5 and ask_tips(miner, pool, mirror) == [3, 4]


def test_twins(miner):
    storm, children = pu.twin_storm(1, 257)
    pool, mirror, _ = feed(miner, [storm], 0)
    with pool:
        table = Table()
        tips = ask_tips(miner, pool, mirror)
        # the lowest twin has the children; every other twin, and every child, is a tip
        assert tips == [0, 1, 2] + list(range(4, 804)) and mirror.parent[children[0]] == 3
        ask_subtrees(miner, pool, mirror, table, [3, 4, 5, children[0], children[-1], 0])
        assert pool.subtrees([3, 5])[0].tolist() == [101, 1]
        survivors = do_drop(miner, pool, mirror, table, storm, [3], 0)  # the lower twin goes, and its children with it
        assert len(mirror) == 703 and mirror.find(pu.name_of(storm[3])) == 3  # the next twin has the name now
        # new children of the dropped name hang on the twin that is left
        _, _, infos = feed(miner, [[storm[children[0]]]], 0, mirror=mirror, pool=pool)
        table.added(infos[0])
        assert mirror.parent[703] == 3 and ask_subtrees(miner, pool, mirror, table, [3]) >= 0
        assert pool.subtrees([3])[0].tolist() == [2]
        r = miner.index_blocks(survivors + [storm[children[0]]], 0)
        assert r.parent.tobytes() == pool.read().parent.tobytes()


def test_hash_flagged_blocks(miner, chain1025):
    """A POW_V_HASH block has no name: nobody's parent, so a tip, and its children are orphans."""
    blocks = [pu.copy_block(b) for b in chain1025[:6]]
    pu.vu.flip_hash_digit(blocks, 2)
    pool, mirror, _ = feed(miner, [blocks], 0)
    with pool:
        table = Table()
        assert mirror.status[2] & 1 and mirror.parent[3] == POOL_NONE
        assert ask_tips(miner, pool, mirror) == [2, 5] and mirror.tips(True) == []
        ask_subtrees(miner, pool, mirror, table, range(6))
        assert pool.subtrees([0, 2, 3])[0].tolist() == [3, 1, 3]
        do_drop(miner, pool, mirror, table, blocks, [2, 2], 0)
        assert len(mirror) == 5 and ask_tips(miner, pool, mirror) == [1, 4]


# ---- after a drop ----
def test_after_a_drop(miner, tree):
    blocks, _ = pu.shuffled(tree, 23)
    pool, mirror, _ = feed(miner, [blocks], pu.D)
    with pool:
        table = Table()
        sizes = mirror.subtrees(range(40))[0]
        root = max((i for i in range(40) if sizes[i] < 20), key=lambda i: sizes[i])  # the largest proper branch
        ask_subtrees(miner, pool, mirror, table, [root])
        assert pool.lift_info()["bytes"] == 4 * 64 * 5
        before = mirror.drop([])  # nothing: the identity, the pool and the table untouched
        assert before == list(range(40))
        new, info = pool.drop([])
        assert new.tolist() == before and info["rehashed"] == 0 and pool.lift_info()["covered"] == 40
        assert miner.stats()["launches"] == 0  # no roots: no GPU work
        survivors = do_drop(miner, pool, mirror, table, blocks, [root, root], pu.D)
        dropped = [b for b in blocks if all(b is not s for s in survivors)]
        assert len(survivors) == 40 - sizes[root] and len(dropped) == sizes[root] > 4
        # a K13 query works afterwards, on a table made again
        pairs, _ = every_query(mirror, extra=1)
        assert ask_forks(miner, pool, mirror, table, pairs) == max((len(mirror) - 1).bit_length() - 1, 0)
        # the dropped blocks come back, children in front of parents
        _, _, infos = feed(miner, [dropped[::-1]], pu.D, mirror=mirror, pool=pool)
        table.added(infos[0])
        r, mine = miner.index_blocks(survivors + dropped[::-1], pu.D), pool.read()
        assert (r.parent.tobytes(), r.depth.tobytes(), r.n_bad.tobytes(), r.status.tobytes(), r.best) == \
            (mine.parent.tobytes(), mine.depth.tobytes(), mine.n_bad.tobytes(), mine.status.tobytes(), mine.best)
        ask_subtrees(miner, pool, mirror, table, range(40))
        ask_tips(miner, pool, mirror)


def test_drop_everything_and_go_on(miner, tree):
    pool, mirror, _ = feed(miner, [tree], pu.D)
    with pool:
        table = Table()
        both = [i for i in range(40) if mirror.parent[i] == POOL_ROOT]
        do_drop(miner, pool, mirror, table, tree, both + both, pu.D)
        assert len(mirror) == 0 and pool.info()["best"] is None
        assert pool.tips().tolist() == [] and miner.stats()["launches"] == 0
        new, info = pool.drop([])
        assert new.tolist() == [] and miner.stats()["launches"] == 0
        feed(miner, [tree[:9]], pu.D, mirror=mirror, pool=pool)
        ask_subtrees(miner, pool, mirror, Table(), range(9))


def test_a_drop_that_changes_the_capacity(miner, chain1025):
    blocks = chain1025[:300]
    pool, mirror, infos = feed(miner, [blocks], 0)
    with pool:
        table = Table()
        assert infos[0]["capacity"] == 512
        do_drop(miner, pool, mirror, table, blocks, [40], 0)
        info = pool.info()
        assert (info["size"], info["capacity"]) == (40, 64)
        ask_subtrees(miner, pool, mirror, table, [0, 39, 20])
        feed(miner, [blocks[40:200]], 0, mirror=mirror, pool=pool)  # and it grows again
        assert pool.info()["capacity"] == 256 and pool.subtrees([0])[0].tolist() == [200]


# ---- the fuzz ----
@pytest.mark.parametrize("seed,difficulty", pu.FUZZ)
def test_fuzz(miner, seed, difficulty):
    blocks = pu.random_pool(seed)
    pool, mirror, _ = feed(miner, [blocks], difficulty)
    with pool:
        table = Table()
        rng = random.Random(seed)
        n = len(mirror)
        ask_tips(miner, pool, mirror)
        ask_subtrees(miner, pool, mirror, table, [rng.randrange(n) for _ in range(64)])
        ask_subtrees(miner, pool, mirror, table, [rng.randrange(n) for _ in range(5)], marks=False)
        sizes = mirror.subtrees(range(min(n, 80)))[0]
        roots = [max(range(len(sizes)), key=lambda i: sizes[i])] + [rng.randrange(n) for _ in range(3)]
        do_drop(miner, pool, mirror, table, blocks, roots, difficulty)
        ask_tips(miner, pool, mirror)
        if len(mirror):
            ask_subtrees(miner, pool, mirror, table, [rng.randrange(len(mirror)) for _ in range(7)])


# ---- the usual refusals ----
def test_an_empty_pool(miner):
    L = miner.L
    with miner.open_pool(pu.D) as pool:
        n_out = ctypes.c_size_t(77)
        word = (ctypes.c_uint32 * 1)(POISON)
        zero = (ctypes.c_uint32 * 1)(0)
        assert L.pow_pool_tips(pool.handle, 0, word, 1, ctypes.byref(n_out)) == 0 and n_out.value == 0 and word[0] == POISON
        assert miner.stats() == {"kernel_ms": 0, "launches": 0, "hashes": 0}
        assert [x.tolist() for x in pool.subtrees([], marks=True)] == [[]] * 5 and miner.stats()["launches"] == 0
        assert L.pow_pool_subtrees(pool.handle, zero, 1, word, None, None, None, None, None) == POW_EINVAL
        assert "root 0 (block 0) past the pool's 0" in last_error(L)
        assert L.pow_pool_drop(pool.handle, zero, 1, word, None) == POW_EINVAL and "past the pool's 0" in last_error(L)
        assert L.pow_pool_drop(pool.handle, None, 0, None, None) == 1 and miner.stats()["launches"] == 0
        assert word[0] == POISON and pool.lift_info() == NOTHING


def test_no_roots_is_no_gpu_work(miner, tree):
    pool, mirror, _ = feed(miner, [tree[:9]], pu.D)
    with pool:
        size, height, best, best_index, on = pool.subtrees([], marks=True)
        assert size.tolist() == [] and on.tolist() == [0] * 9
        assert miner.stats() == {"kernel_ms": 0, "launches": 0, "hashes": 0} and pool.lift_info() == NOTHING


def test_a_context_bound_to_a_stop_board_refuses_the_calls(tree):
    with GpuMiner(0) as m, StopBoard(2) as board:
        L = m.L
        pool, mirror, _ = feed(m, [tree[:5]], pu.D)
        with pool:
            m.bind_board(board, 0, 1)
            try:
                words = (ctypes.c_uint32 * 5)(*[POISON] * 5)
                n_out = ctypes.c_size_t(77)
                at = (ctypes.c_uint32 * 1)(4)
                assert L.pow_pool_tips(pool.handle, 0, words, 5, ctypes.byref(n_out)) == POW_EINVAL
                assert "pow_pool_tips does not run on a context bound to a stop board" in last_error(L)
                assert L.pow_pool_subtrees(pool.handle, at, 1, words, None, None, None, None, ctypes.byref(n_out)) == POW_EINVAL
                assert "pow_pool_subtrees does not run on a context bound to a stop board" in last_error(L)
                assert L.pow_pool_drop(pool.handle, at, 1, words, None) == POW_EINVAL
                assert "pow_pool_drop does not run on a context bound to a stop board" in last_error(L)
                assert list(words) == [POISON] * 5 and n_out.value == 77
            finally:
                m.bind_board(None)
            compare(pool, mirror)
            table = Table()
            ask_subtrees(m, pool, mirror, table, range(5))  # unbound: as before
            do_drop(m, pool, mirror, table, tree[:5], [4], pu.D)


def test_a_closed_pool_is_not_touched(miner, tree):
    pool, mirror, _ = feed(miner, [tree[:5]], pu.D)
    pool.close()
    for call in (lambda: pool.subtrees([0]), lambda: pool.drop([0])):
        with pytest.raises(PowError, match="null"):
            call()
    n_out = ctypes.c_size_t(77)
    word = (ctypes.c_uint32 * 1)(POISON)
    assert miner.L.pow_pool_tips(pool.handle, 0, word, 1, ctypes.byref(n_out)) == POW_EINVAL
    assert "null pool" in last_error(miner.L) and word[0] == POISON and n_out.value == 77
