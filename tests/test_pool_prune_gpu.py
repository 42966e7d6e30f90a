"""pow_pool_mark and pow_pool_prune on the GPU against their host statement
(block.BlockPool.mark and .prune, which tests/test_pool_prune_host.py holds
against block.index_blocks).  After every call the whole pool is compared with
the mirror; after every prune also with pow_index_blocks over the surviving
structs, pow_pool_find over the survivors' and the dropped names, and the
launches with the plan's.  The pools are pool_util's, built on the CPU with
hashlib, so the largest has 65,537 blocks (257 partials): the scan's cross-wave
half, rounds 18 to 20 and 4,096 workgroups are in tests/test_pool_deep_gpu.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from mpi_blockchain_amd._lib import PKG, POW_EINVAL, Block, PoolInfo
from mpi_blockchain_amd.block import POOL_NONE, POOL_ROOT, V_INDEX, V_LINK, BlockPool, prune_structs
from mpi_blockchain_amd.miner import GpuMiner, StopBoard

import helpers
import pool_util as pu
import verify_util as vu
from test_pool_stream_gpu import POISON, compare, feed, last_error

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def plan_launches(size: int, kept: int, prune: bool) -> int:
    """pow_pool_prune_launches (csrc/pow_host.cpp): K12a, the rounds, K12c, K12d; a prune that drops and keeps adds
    K12e, K12f and K10b."""
    if size == 0:
        return 0
    return 3 + (size - 1).bit_length() + (3 if prune and 0 < kept < size else 0)


def mark_both(miner, pool, mirror, seeds):
    """pow_pool_mark against the mirror's; the pool's answers stay byte for byte."""
    tips, min_index, sound_only = seeds
    before, info = pool.read(), pool.info()
    on = pool.mark(tips, min_index, sound_only)
    s = miner.stats()
    want = mirror.mark(tips, min_index, sound_only)
    assert on.dtype == np.uint8 and on.tolist() == want
    assert (s["launches"], s["hashes"]) == (plan_launches(len(mirror), sum(want), False), 0)
    assert (s["kernel_ms"] > 0) == (len(mirror) > 0)
    after = pool.read()
    for a, b in ((before.status, after.status), (before.parent, after.parent), (before.depth, after.depth),
                 (before.n_bad, after.n_bad)):
        assert a.tobytes() == b.tobytes()
    assert pool.info() == info
    return want


def prune_both(miner, pool, mirror, structs, seeds):
    """pow_pool_prune against the mirror's, then the pool against the mirror,
    against pow_index_blocks over the survivors and pow_pool_find; returns
    (the surviving structs, the map, the info)."""
    tips, min_index, sound_only = seeds
    size, before = len(mirror), pool.info()
    assert len(structs) == size
    new, info = pool.prune(tips, min_index, sound_only)
    s = miner.stats()
    want = mirror.prune(tips, min_index, sound_only)
    kept = len(mirror)
    assert new.dtype == np.uint32 and new.tolist() == want
    assert (s["launches"], s["hashes"]) == (plan_launches(size, kept, True), 0), (s, size, kept)
    assert (s["kernel_ms"] > 0) == (size > 0)
    assert info["ok"] == mirror.ok and (info["adopted"], info["reranked"]) == (0, 0)
    assert info["rehashed"] == int(kept < size)
    if kept == size:  # nothing is touched
        assert (info["capacity"], info["slots"]) == (before["capacity"], before["slots"])
    else:
        assert info["capacity"] <= before["capacity"] and info["capacity"] & (info["capacity"] - 1) == 0
    compare(pool, mirror)
    assert pool.info() == {k: v for k, v in info.items() if k != "ok"}
    survivors = prune_structs(structs, want)
    dropped = [pu.name_of(b) for b, j in zip(structs, want) if j == POOL_NONE]
    against_index_blocks(miner, pool, mirror, survivors, dropped)
    return survivors, want, info


def against_index_blocks(miner, pool, mirror, structs, dropped=()):
    """The pool against one pow_index_blocks call over `structs` at its
    difficulty, and pow_pool_find of every struct's and every dropped name."""
    r = pool.read()
    if structs:
        ref = miner.index_blocks(structs, mirror.difficulty)
        for a, b in ((r.status, ref.status), (r.parent, ref.parent), (r.depth, ref.depth), (r.n_bad, ref.n_bad)):
            assert a.tobytes() == b.tobytes()
        assert (r.best, r.ok) == (ref.best, ref.ok)
    else:
        assert r.best is None and r.ok and len(r.status) == 0
    names = [pu.name_of(b) for b in structs] + list(dropped)
    assert pool.find(names) == [mirror.find(x) for x in names]


@pytest.fixture(scope="module")
def miner():
    with GpuMiner(0) as m:
        yield m


@pytest.fixture(scope="module")
def smallest():
    """The test library with the smallest first table and a first capacity of one block."""
    with helpers.hooked_miner(("POW_POOL_SLOTS_LOG2", "POW_POOL_FIRST_CAP"), POW_POOL_SLOTS_LOG2=1,
                              POW_POOL_FIRST_CAP=1) as m:
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


# ---- the tree of 40 ----
def forged(tree):
    """The tree with a 41st block: a child of the trunk's tip whose index is
    far too high (V_INDEX), so that the index rule alone would keep it."""
    b = pu.mine_chain(tree[12], 1, pu.D, owner=8, created_at=[1_700_000_999])[0]
    b.index += 1024  # bytes that are not hashed: still sealed, but it no longer follows its parent
    return list(tree) + [b]


TREE_CASES = {
    "tips_only": ("tree", ([25, 39], None, False), 22),           # the race's tip and the second root's chain
    "duplicate_tips": ("tree", ([31, 31, 12, 31], None, False), 17),  # the top branch twice over, and the trunk's tip
    "index_only": ("tree", ([], 14, False), None),
    "index_and_tips": ("tree", ([27], 15, True), None),
    "sound_only_drops_the_forged_block": ("forged", ([], 16, True), None),
    "the_forged_block_as_a_tip_stays": ("forged", ([40], 16, True), None),
    "min_index_0_keeps_everything": ("tree", ([], 0, False), 40),
    "min_index_all_ones_keeps_nothing": ("tree", ([], 0xFFFFFFFF, False), 0),
    "nothing_marked": ("tree", ([], None, True), 0),
    "everything_marked_by_tips": ("tree", ([20, 25, 26, 27, 31, 39], None, False), 40),
}


@pytest.mark.parametrize("case", sorted(TREE_CASES))
def test_tree(miner, tree, case):
    which, seeds, kept = TREE_CASES[case]
    blocks = forged(tree) if which == "forged" else list(tree)
    pool, mirror, _ = feed(miner, [blocks[:17], blocks[17:]], pu.D)
    with pool:
        if which == "forged":
            assert mirror.status[40] == V_INDEX and mirror.index[40] == 1038 and mirror.n_bad[40] == 1
        on = mark_both(miner, pool, mirror, seeds)
        survivors, new, info = prune_both(miner, pool, mirror, blocks, seeds)
        assert sum(on) == len(survivors) == info["size"] and (kept is None or kept == len(survivors))
        if case == "sound_only_drops_the_forged_block":
            assert new[40] == POOL_NONE and 0 < len(survivors) < 40
        if case == "the_forged_block_as_a_tip_stays":
            assert new[40] == len(survivors) - 1 and not info["ok"] and new[12] != POOL_NONE
        if kept == 0:
            assert info["best"] is None and info["n_flagged"] == 0 and info["capacity"] == 64 and info["slots"] == 128
        if kept == 40:
            assert new == list(range(40)) and info["rehashed"] == 0
        # adds go on at the new positions: the race's next block, then a block of a fork that may be gone
        more = [pu.mine_chain(tree[25], 1, pu.D, owner=3, created_at=[1_700_000_777])[0],
                pu.mine_chain(tree[27], 1, pu.D, owner=4, created_at=[1_700_000_778])[0]]
        feed(miner, [[b] for b in more], pu.D, mirror=mirror, pool=pool)
        survivors = survivors + more
        against_index_blocks(miner, pool, mirror, survivors)
        for b, at in zip(more, (25, 27)):
            j = len(survivors) - 2 + more.index(b)
            if new[at] == POOL_NONE:  # its parent was dropped: an orphan, as in that pow_index_blocks call
                assert mirror.parent[j] == POOL_NONE and mirror.status[j] & V_LINK
            else:
                assert mirror.parent[j] == new[at]


def test_an_empty_pool_does_no_gpu_work(miner, tree):
    with miner.open_pool(pu.D) as pool:
        mirror = BlockPool(pu.D)
        assert mark_both(miner, pool, mirror, ([], 0, False)) == []
        survivors, new, info = prune_both(miner, pool, mirror, [], ([], 0, False))
        assert new == [] and info["size"] == 0 and info["best"] is None  # prune_both has held the launches against 0
        feed(miner, [tree[:5]], pu.D, mirror=mirror, pool=pool)


# ---- depth seams of the rounds ----
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("n", [512, 513, 1025])
def test_one_seed_at_the_tip_marks_the_whole_chain(miner, chain1025, n, reverse):
    """A walk of n blocks under the one seed: ceil(log2 n) rounds reach the
    root, one fewer would leave it unmarked."""
    chain = chain1025[:n]
    blocks = chain[::-1] if reverse else chain
    tip = 0 if reverse else n - 1
    pool, mirror, _ = feed(miner, [blocks], 0, reserve=n)
    with pool:
        assert mirror.depth[tip] == n and mirror.ok
        on = mark_both(miner, pool, mirror, ([tip], None, False))
        assert on == [1] * n
        root = n - 1 if reverse else 0
        below = mark_both(miner, pool, mirror, ([mirror.parent[mirror.parent[tip]]], None, False))
        assert sum(below) == n - 2 and below[root] == 1 and below[tip] == 0
        survivors, new, info = prune_both(miner, pool, mirror, blocks, ([tip], None, False))
        assert new == list(range(n)) and info["rehashed"] == 0 and info["size"] == n


# ---- workgroup and wave seams of count, scan and gather ----
def braided(main, side):
    """main and side by turns while both last, then the rest: kept and dropped
    blocks alternate across every wave boundary the shorter one reaches."""
    out, where = [], []
    for k in range(max(len(main), len(side))):
        for part, flag in ((main, 1), (side, 0)):
            if k < len(part):
                out.append(part[k])
                where.append(flag)
    return out, where


@pytest.mark.parametrize("size,kept", [(size, kept) for size in (257, 511, 513, 1025)
                                       for kept in (63, 64, 65, 255, 256, 257)])
def test_kept_counts_at_the_seams(miner, chain1025, side, size, kept):
    """257 of 257 is the prune that drops nothing."""
    main = chain1025[:kept]
    blocks, where = braided(main, side[:size - kept])
    tip = len(blocks) - 1 - where[::-1].index(1)
    assert len(blocks) == size and blocks[tip] is main[-1]
    pool, mirror, _ = feed(miner, [blocks], 0)
    with pool:
        on = mark_both(miner, pool, mirror, ([tip], None, False))
        assert on == where
        survivors, new, info = prune_both(miner, pool, mirror, blocks, ([tip], None, False))
        assert len(survivors) == kept and survivors == main and info["best"] == kept - 1 and info["ok"]
        assert info["capacity"] == max(64, 1 << (kept - 1).bit_length())


def test_a_pool_across_the_host_tile_seam_half_dropped(miner):
    """65,537 blocks at d = 0: 257 partials for the scan, two tiles for the
    add.  Two chains by turns, one of them kept: a walk of 32,769 blocks
    under the one seed, and every other block dropped."""
    n = vu.HOST_TILE + 1
    a, b = pu.flat_chain(n // 2 + 1, 0, seed=201), pu.flat_chain(n // 2, 0, seed=202)
    blocks, where = braided(a, b)
    assert len(blocks) == n == 65537 and where[-1] == 1
    pool, mirror, _ = feed(miner, [blocks], 0, reserve=n)
    with pool:
        on = mark_both(miner, pool, mirror, ([n - 1], None, False))
        assert on == where and sum(on) == 32769
        survivors, new, info = prune_both(miner, pool, mirror, blocks, ([n - 1], None, False))
        assert len(survivors) == 32769 and info["capacity"] == 65536 and info["slots"] == 131072
        assert info["best"] == 32768 and info["best_index"] == 32769


# ---- twins ----
@pytest.mark.parametrize("low_index,other_index", [(1, 257), (257, 1)])
def test_twins(miner, low_index, other_index):
    storm, children = pu.twin_storm(low_index, other_index)
    name = pu.name_of(storm[3])
    # a higher twin is a seed while the lowest is not: the name passes to the lowest twin that is kept
    pool, mirror, _ = feed(miner, [storm], 0)
    with pool:
        assert pool.find([name]) == [3]
        survivors, new, info = prune_both(miner, pool, mirror, storm, ([500, 700, 5], None, False))
        assert new[3] == POOL_NONE and (new[5], new[500], new[700]) == (0, 1, 2) and pool.find([name]) == [0]
        feed(miner, [[storm[children[0]]]], 0, mirror=mirror, pool=pool)  # a child finds the lowest twin kept
        assert mirror.parent[3] == 0
        against_index_blocks(miner, pool, mirror, survivors + [storm[children[0]]])
    # the lowest twin is kept as a child's parent, beside a higher twin that is a seed
    pool, mirror, _ = feed(miner, [storm], 0)
    with pool:
        survivors, new, info = prune_both(miner, pool, mirror, storm, ([children[50], 5, children[99]], None, False))
        assert info["size"] == 4 and new[3] == 0 and mirror.parent == [POOL_ROOT, POOL_ROOT, 0, 0]
        assert pool.find([name]) == [0]


# ---- orphans ----
def test_a_kept_orphan_is_adopted_after_the_prune(miner, tree):
    blocks = tree[2:13] + tree[33:]  # the trunk on a parent that is not there, and a chain whose root is not there
    pool, mirror, _ = feed(miner, [blocks], pu.D)
    with pool:
        survivors, new, info = prune_both(miner, pool, mirror, blocks, ([10], None, False))
        assert info["size"] == 11 and mirror.parent[0] == POOL_NONE and not info["ok"] and info["best"] is None
        _, _, infos = feed(miner, [[tree[1]], [tree[0]]], pu.D, mirror=mirror, pool=pool)
        assert [(i["adopted"], i["reranked"]) for i in infos] == [(1, 1), (1, 1)]
        assert infos[-1]["ok"] and infos[-1]["best"] == 10 and mirror.depth[10] == 13
        survivors = survivors + [tree[1], tree[0]]
        against_index_blocks(miner, pool, mirror, survivors)
        # a child that arrives after its parent was dropped
        _, _, infos = feed(miner, [[tree[35]]], pu.D, mirror=mirror, pool=pool)
        assert mirror.parent[-1] == POOL_NONE and mirror.status[-1] == V_LINK and infos[0]["adopted"] == 0
        against_index_blocks(miner, pool, mirror, survivors + [tree[35]])


# ---- prune, add, prune again ----
def test_capacity_shrinks_and_grows_again(smallest, chain1025, side):
    """The test library from one block and two slots: every add and every
    prune leaves slots >= 2 size (compare() checks it) at the lowest power of
    two, and the capacity follows the pool down and up."""
    miner = smallest
    blocks, where = braided(chain1025[:300], side[:300])
    pool, mirror, infos = feed(miner, [blocks[:200], blocks[200:]], 0)
    with pool:
        assert infos[-1]["capacity"] == 1024 and infos[-1]["slots"] == 2048
        tip = len(blocks) - 2
        assert where[tip] == 1
        structs, new, info = prune_both(miner, pool, mirror, blocks, ([mirror.parent[mirror.parent[tip]]], None, False))
        assert (info["size"], info["capacity"], info["slots"]) == (298, 512, 1024)
        structs, new, info = prune_both(miner, pool, mirror, structs, ([2], None, False))
        assert (info["size"], info["capacity"], info["slots"]) == (3, 4, 8)
        _, _, infos = feed(miner, [[chain1025[3]], chain1025[4:6], chain1025[298:300], chain1025[6:40]], 0,
                           mirror=mirror, pool=pool)
        structs = structs + chain1025[3:6] + chain1025[298:300] + chain1025[6:40]
        assert [(i["size"], i["capacity"], i["slots"], i["rehashed"]) for i in infos] == \
            [(4, 4, 8, 0), (6, 8, 16, 1), (8, 8, 16, 0), (42, 64, 128, 1)]
        against_index_blocks(miner, pool, mirror, structs)
        structs, new, info = prune_both(miner, pool, mirror, structs, ([], 39, True))  # the two orphans go
        assert (info["size"], info["capacity"], info["slots"], info["best_index"]) == (40, 64, 128, 40)
        structs, new, info = prune_both(miner, pool, mirror, structs, ([0], None, False))
        assert (info["size"], info["capacity"], info["slots"]) == (1, 1, 2)
        structs, new, info = prune_both(miner, pool, mirror, structs, ([], None, False))
        assert (info["size"], info["capacity"], info["slots"], info["best"]) == (0, 1, 2, None)
        feed(miner, [chain1025[:3]], 0, mirror=mirror, pool=pool)
        against_index_blocks(miner, pool, mirror, chain1025[:3])


@pytest.mark.parametrize("seed,difficulty", pu.FUZZ[:4])
def test_fuzz(miner, seed, difficulty):
    blocks = pu.random_pool(seed)
    pool, mirror, _ = feed(miner, [blocks[:150], blocks[150:]], difficulty)
    with pool:
        top = max(mirror.index)
        seeds = ([7, len(blocks) - 1, 7], top - 4, bool(seed & 1))
        mark_both(miner, pool, mirror, seeds)
        structs, new, info = prune_both(miner, pool, mirror, blocks, seeds)
        assert 0 < info["size"] < len(blocks)
        more = pu.random_pool(seed + 1000)[:40] + blocks[:30]  # strangers, and blocks that were there before
        feed(miner, [more[:35], more[35:]], difficulty, mirror=mirror, pool=pool)
        structs = structs + more
        against_index_blocks(miner, pool, mirror, structs)
        prune_both(miner, pool, mirror, structs, ([], max(mirror.index) - 2, False))


# ---- mark between adds ----
def test_mark_between_adds_leaves_the_adds_as_they_are(miner, tree):
    """feed() holds every add's launches against the add's own plan: a mark in
    between (whose scratch the add's rounds use too) changes none of them."""
    pool = mirror = None
    try:
        for lo in range(0, 40, 8):
            pool, mirror, infos = feed(miner, [tree[lo:lo + 8]], pu.D, mirror=mirror, pool=pool)
            assert infos[0]["reranked"] == 0 and miner.stats()["launches"] == 4 + 3
            mark_both(miner, pool, mirror, ([mirror.best], None, False))
            mark_both(miner, pool, mirror, ([], max(mirror.index) - 1, True))
    finally:
        if pool is not None:
            pool.close()


# ---- the calls' refusals ----
def test_einval_in_the_stated_order_on_a_live_pool(miner, tree):
    """Each case has every LATER fault too, and the message names the first.
    Nothing is written; the pool, its info and the context's stats stay."""
    L = miner.L
    pool, mirror, _ = feed(miner, [tree[:5]], pu.D)
    with pool:
        stats = miner.stats()
        info = PoolInfo(*[POISON] * 9)
        words = (ctypes.c_uint32 * 5)(*[POISON] * 5)
        n_on = ctypes.c_size_t(77)
        past = (ctypes.c_uint32 * 3)(0, 5, 4)
        never_read = ctypes.cast(ctypes.c_void_p(8), ctypes.POINTER(ctypes.c_uint32))
        calls = (lambda tips, k, flags: L.pow_pool_mark(pool.handle, tips, k, 0, flags, words, ctypes.byref(n_on)),
                 lambda tips, k, flags: L.pow_pool_prune(pool.handle, tips, k, 0, flags, words, ctypes.byref(info)))
        for call in calls:
            for flags in (4, 7, 0x80000000):
                assert call(None, (1 << 16) + 1, flags) == POW_EINVAL and "unknown flags" in last_error(L)
            for k in ((1 << 16) + 1, 1 << 40):
                assert call(None, k, 3) == POW_EINVAL and "too many tips" in last_error(L)
                assert call(never_read, k, 0) == POW_EINVAL and "too many tips" in last_error(L)
            assert call(None, 1, 3) == POW_EINVAL and "null tips" in last_error(L)
            assert call(None, 1 << 16, 0) == POW_EINVAL and "null tips" in last_error(L)
            assert call(past, 3, 1) == POW_EINVAL and "tip 1 (block 5) past the pool's 5" in last_error(L)
        assert [getattr(info, n) for n, _ in PoolInfo._fields_] == [POISON] * 9 and list(words) == [POISON] * 5
        assert n_on.value == 77 and pool.info()["size"] == 5 and miner.stats() == stats
        compare(pool, mirror)
        # null outputs are allowed
        assert L.pow_pool_mark(pool.handle, past, 1, 0, 0, None, None) == 0
        assert L.pow_pool_prune(pool.handle, None, 0, 0, 1, None, None) == 1  # everything marked
        compare(pool, mirror)
        feed(miner, [tree[5:9]], pu.D, mirror=mirror, pool=pool)


def test_a_context_bound_to_a_stop_board_refuses_both_calls(tree):
    with GpuMiner(0) as m, StopBoard(2) as board:
        L = m.L
        pool, mirror, _ = feed(m, [tree[:5]], pu.D)
        with pool:
            m.bind_board(board, 0, 1)
            try:
                info = PoolInfo(*[POISON] * 9)
                words = (ctypes.c_uint32 * 5)(*[POISON] * 5)
                tips = (ctypes.c_uint32 * 1)(4)
                assert L.pow_pool_mark(pool.handle, tips, 1, 0, 0, words, None) == POW_EINVAL
                assert "pow_pool_mark does not run on a context bound to a stop board" in last_error(L)
                assert L.pow_pool_prune(pool.handle, tips, 1, 0, 0, words, ctypes.byref(info)) == POW_EINVAL
                assert "pow_pool_prune does not run on a context bound to a stop board" in last_error(L)
                assert info.size == POISON and list(words) == [POISON] * 5
            finally:
                m.bind_board(None)
            compare(pool, mirror)
            prune_both(m, pool, mirror, tree[:5], ([3], None, False))  # unbound: as before


# ---- the example ----
def test_c_example(tmp_path):
    """examples/pool_prune.c builds against the shipped library and runs: what
    it prints is what the mirror says over the pool it dumped."""
    exe, dump = str(tmp_path / "pool_prune"), str(tmp_path / "pool.bin")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "pool_prune.c"), "-L", PKG, "-lpow_gpu",
                    f"-Wl,-rpath,{PKG}", "-o", exe], check=True)
    p = subprocess.run([exe, "10", "9", dump], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    raw = open(dump, "rb").read()
    n = 1 + 3 * 10  # the published shape: 3 rivals x 10 heights on a root
    assert len(raw) == (n + 1) * ctypes.sizeof(Block)
    blocks = list((Block * (n + 1)).from_buffer_copy(raw))
    mirror = BlockPool(9)
    mirror.add(blocks[:n])
    line = (r"size (\d+) flagged (\d+) best (-?\d+) index (\d+) rehashed (\d+) capacity (\d+) slots (\d+); "
            r"(\d+) launches$")
    fed = re.search(r"^fed: " + line, p.stdout, flags=re.M)
    assert [int(x) for x in fed.groups()] == [n, 0, mirror.best, 10, 0, 64, 128, 1 + 3 + 5]
    tip = mirror.best
    assert f"chain under block {tip}: 11 blocks; {plan_launches(n, 11, False)} launches" in p.stdout
    assert sum(mirror.mark([tip])) == 11
    new = mirror.prune([], 5, True)
    kept = len(mirror)
    assert kept == 5 + 3 * 6  # the winners below index 5, and every rival from there on
    pruned = re.search(r"^pruned from index 5: kept: " + line, p.stdout, flags=re.M)
    assert [int(x) for x in pruned.groups()] == [kept, 0, new[tip], 10, 1, 64, 128, plan_launches(n, kept, True)]
    mirror.add([blocks[n]])
    nxt = re.search(r"^next block: " + line, p.stdout, flags=re.M)
    assert [int(x) for x in nxt.groups()] == [kept + 1, 0, kept, 11, 0, 64, 128, 4]
    assert mirror.best == kept and mirror.parent[kept] == new[tip] and mirror.depth[kept] == 12
    b = blocks[n]
    assert (f"block 11 at {kept} owner 0 nonce {b.nonce.decode()} hash {b.block_hash.decode()} "
            f"parent {new[tip]} depth 12") in p.stdout
    assert f"pool of {n} blocks pruned to {kept} and fed again at difficulty 9" in p.stdout
