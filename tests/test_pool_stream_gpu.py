"""pow_pool on the GPU against its host statement (block.BlockPool, which
tests/test_pool_stream_host.py holds against block.index_blocks): after every
add the four per-block results, the fork choice, the flagged count, the
adopted count, which path the add took and its launches.  The pools are
pool_util's, built on the CPU with hashlib."""
import ctypes
import random

import numpy as np
import pytest

from mpi_blockchain_amd._lib import POW_EHIP, POW_EINVAL, Block, PoolInfo, PowError
from mpi_blockchain_amd.block import POOL_NONE, V_HASH, BlockPool, index_blocks
from mpi_blockchain_amd.miner import GpuMiner, StopBoard

import helpers
import pool_util as pu
import verify_util as vu
from test_pool_gpu import PREV_RULES
from test_pool_stream_host import batches_of

pytestmark = pytest.mark.gpu

T = vu.HOST_TILE


def launches(m: int, size: int, reranked: bool) -> int:
    """The header's: what pow_index_blocks takes on the m blocks alone, and on a re-rank K11s and K10c to K10e."""
    return pu.launches(m) + (3 + (size - 1).bit_length() if reranked else 0)


def compare(pool, mirror: BlockPool):
    """The pool's whole state against the mirror's."""
    n = len(mirror)
    r, info = pool.read(), pool.info()
    assert r.status.dtype == np.uint8 and np.array_equal(r.status, np.array(mirror.status, dtype=np.uint8))
    for got, want in ((r.parent, mirror.parent), (r.depth, mirror.depth), (r.n_bad, mirror.n_bad)):
        assert got.dtype == np.uint32 and np.array_equal(got, np.array(want, dtype=np.uint32))
    assert (info["size"], info["n_flagged"], info["best"]) == (n, mirror.n_flagged, mirror.best)
    assert info["best_index"] == (0 if mirror.best is None else mirror.index[mirror.best])
    assert r.best == mirror.best and r.ok == mirror.ok
    assert info["capacity"] >= n and info["slots"] >= 2 * n and info["slots"] & (info["slots"] - 1) == 0


def feed(miner, batches, difficulty, reserve=0, mirror=None, pool=None):
    """Every batch into a pool (a new one unless given) and into the mirror,
    everything compared after every add; returns (pool, mirror, the adds' infos)."""
    pool = miner.open_pool(difficulty, reserve) if pool is None else pool
    mirror = BlockPool(difficulty) if mirror is None else mirror
    infos = []
    for batch in batches:
        mirror.add(batch)
        info = pool.add(batch)
        s = miner.stats()
        assert info["ok"] == mirror.ok
        assert (info["adopted"], info["reranked"]) == (mirror.adopted, int(mirror.adopted > 0))
        assert s["hashes"] == len(batch) and s["launches"] == launches(len(batch), len(mirror), mirror.adopted > 0)
        assert s["kernel_ms"] > 0
        compare(pool, mirror)
        infos.append(info)
    return pool, mirror, infos


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
def chain513():
    return pu.flat_chain(513, 0, seed=77)


# ---- arrival order ----
def test_tree_in_mining_order_never_re_ranks(miner, tree):
    pool, mirror, infos = feed(miner, [[b] for b in tree], pu.D)
    with pool:
        assert [(i["adopted"], i["reranked"]) for i in infos] == [(0, 0)] * 40
        assert miner.stats()["launches"] == 4 and mirror.ok and infos[-1]["ok"]
        assert pool.add([])["size"] == 40 and miner.stats()["launches"] == 0  # m = 0 changes nothing
        compare(pool, mirror)
        assert len(pool) == 40


def test_tree_reversed_adopts_with_every_parent(miner, tree):
    blocks = tree[::-1]
    pool, mirror, infos = feed(miner, [[b] for b in blocks], pu.D)
    with pool:
        parent = index_blocks(blocks, pu.D)[1]
        assert [i["reranked"] for i in infos] == [int(k in parent) for k in range(40)]
        assert sum(i["adopted"] for i in infos) == 38 and infos[-1]["ok"]  # every block but the two roots


@pytest.mark.parametrize("size", [1, 2, 3, 7, 27])
def test_tree_shuffled_in_batches(miner, tree, size):
    blocks, _ = pu.shuffled(tree, 40 + size)
    pool, mirror, infos = feed(miner, batches_of(blocks, (size,)), pu.D)
    pool.close()
    assert any(i["reranked"] for i in infos) and mirror.ok


# ---- workgroup and wave seams ----
@pytest.mark.parametrize("swapped", [False, True])
@pytest.mark.parametrize("sizes", [(255, 1, 1, 256), (63, 1, 1, 448)])
def test_chain_across_the_seams(miner, chain513, sizes, swapped):
    parts = batches_of(chain513, sizes)
    assert [len(p) for p in parts] == list(sizes)
    if swapped:  # the upper half first: its lowest block is an orphan until the last add
        parts = parts[::-1]
    pool, mirror, infos = feed(miner, parts, 0)
    pool.close()
    assert [i["adopted"] for i in infos] == ([0, 1, 1, 1] if swapped else [0] * 4)
    assert mirror.ok and max(mirror.depth) == 513 and mirror.index[mirror.best] == 513


# ---- growth ----
def test_growth_of_arrays_and_table(smallest, chain513):
    """reserve 0 from one block and two slots, in batches of 50: the info
    counters say when the arrays doubled and when the table was rebuilt."""
    pool, mirror, infos = feed(smallest, batches_of(chain513, (50,)), 0)
    pool.close()
    cap, slots, n = 1, 2, 0
    for info in infos:
        n = min(n + 50, 513)
        while cap < n:
            cap *= 2
        rebuilt = n > slots // 2
        if rebuilt:
            slots = 1 << (2 * n - 1).bit_length()
        assert (info["capacity"], info["slots"], info["rehashed"]) == (cap, slots, int(rebuilt)), info
    assert [i["capacity"] for i in infos] == [64, 128, 256, 256, 256, 512, 512, 512, 512, 512, 1024]
    assert sum(i["rehashed"] for i in infos) == 5 and infos[-1]["slots"] == 2048


@pytest.mark.parametrize("reserve", [0, 513, 4096])
@pytest.mark.parametrize("hooked", [False, True])
def test_results_do_not_depend_on_reserve_or_the_switches(miner, smallest, chain513, reserve, hooked):
    blocks, _ = pu.shuffled(chain513, 3)
    pool, mirror, infos = feed(smallest if hooked else miner, batches_of(blocks, (50,)), 0, reserve=reserve)
    pool.close()
    if reserve:
        assert infos[0]["capacity"] == reserve
    elif hooked:
        assert infos[0]["capacity"] == 64  # from the switch's one block, doubled until it holds the first 50
    else:
        assert infos[0]["capacity"] == 64  # the shipped first capacity, which holds them as it is
    assert mirror.ok and any(i["reranked"] for i in infos)
    if reserve:
        assert len({i["capacity"] for i in infos}) == 1


def test_default_first_capacity_doubles_to_1024(miner, chain513):
    pool, _, infos = feed(miner, batches_of(chain513 + pu.flat_chain(511, 0, seed=78), (128,)), 0)
    pool.close()
    assert [i["capacity"] for i in infos] == [128, 256, 512, 512, 1024, 1024, 1024, 1024]  # from 64


# ---- twins ----
@pytest.mark.parametrize("low_index,other_index", [(1, 257), (257, 1)])
def test_a_late_twin_does_not_take_the_name(miner, low_index, other_index):
    storm, children = pu.twin_storm(low_index, other_index)
    blocks = storm[:3] + storm[4:] + [storm[3]]  # the twin of position 3 comes last, alone
    pool, mirror, infos = feed(miner, [blocks[:803], blocks[803:]], 0)
    pool.close()
    assert {mirror.parent[k - 1] for k in children} == {3} and mirror.parent[803] == 0xFFFFFFFF
    assert infos[1]["adopted"] == 0 and mirror.index[3] == other_index


@pytest.mark.parametrize("reserve", [0, 1024])  # the twins through K10b on a rebuild, and through K11b
def test_a_hundred_orphans_adopted_in_one_add(miner, reserve):
    storm, children = pu.twin_storm(1, 257)
    rest = [b for k, b in enumerate(storm) if k not in set(children)]
    pool, mirror, infos = feed(miner, [[storm[k] for k in children], rest], 0, reserve=reserve)
    pool.close()
    assert infos[1]["rehashed"] == (0 if reserve else 1)
    assert infos[0]["n_flagged"] == 100 and (infos[1]["adopted"], infos[1]["reranked"]) == (100, 1)
    assert {mirror.parent[k] for k in range(100)} == {103} and mirror.ok


def test_twins_race_for_their_slot_inside_one_batch(miner):
    """64 digests, each held by a block in the last lane of workgroup g of the
    insert and by eight twins in an early lane of the eight workgroups after
    it: whichever takes the slot first, the lowest position keeps the name
    (K11b's atomicMin).  Nothing rebuilds the table here, so the batch goes
    through K11b; the children, added afterwards, say who holds each name."""
    groups, filler = 64, pu.genesis(900, 0)
    batch = [filler] * ((groups + 8) * 256)
    children = []
    for g in range(groups):
        r, c = pu.flat_chain(2, 0, seed=1000 + g)
        low = pu.copy_block(r)
        low.index += 256  # not hashed: the same digest, and the child's index no longer fits
        batch[g * 256 + 255] = low
        for k in range(1, 9):
            batch[(g + k) * 256 + g] = r
        children.append(c)
    pool, mirror, infos = feed(miner, [batch, children], 0, reserve=1 << 15)
    pool.close()
    assert [i["rehashed"] for i in infos] == [0, 0]
    assert mirror.parent[len(batch):] == [g * 256 + 255 for g in range(groups)]
    assert mirror.status[len(batch):] == [8] * groups  # V_INDEX against the low twin


# ---- names ----
def test_only_the_untampered_name_adopts():
    sweep, _ = pu.name_sweep()
    blocks = sweep[1:1021] + [sweep[0]]  # the tampered children of the name's positions 0-3, then the root
    with GpuMiner(0) as m:
        pool, mirror, infos = feed(m, [blocks[:1020], blocks[1020:]], 0)
        pool.close()
    assert (infos[1]["adopted"], infos[1]["reranked"]) == (0, 0)
    assert mirror.parent[1:1020] == [POOL_NONE] * 1019 and mirror.parent[0] == 0xFFFFFFFF  # NUL at 0: the empty string


# ---- the host-tile seam ----
@pytest.fixture(scope="module")
def seam():
    """test_pool_gpu.test_host_tile_seam's list and its mirror computation."""
    n = T + 1
    c = vu.build_chain(n, 0, seed=8)
    vu.flip_hash_digit(c, n // 2)
    rows = np.frombuffer(c, dtype=np.uint8).reshape(n, ctypes.sizeof(Block))
    perm = np.random.default_rng(9).permutation(n)
    raw = np.ascontiguousarray(rows[perm])
    return raw, index_blocks((Block * n).from_buffer_copy(raw.tobytes()), 0)


@pytest.mark.parametrize("first", [T, 1])
def test_host_tile_seam(miner, seam, first):
    raw, (status, parent, depth, n_bad, best) = seam
    n = T + 1
    parts = [(Block * k).from_buffer_copy(raw[lo:lo + k].tobytes()) for lo, k in ((0, first), (first, n - first))]
    with miner.open_pool(0, reserve=n) as pool:
        a = pool.add(parts[0])
        assert miner.stats()["launches"] == launches(first, first, False) and a["adopted"] == 0
        b = pool.add(parts[1])
        late = sum(1 for i in range(first) if parent[i] != POOL_NONE and parent[i] < n and parent[i] >= first)
        assert (b["adopted"], b["reranked"]) == (late, int(late > 0))
        assert miner.stats()["launches"] == launches(n - first, n, late > 0) and miner.stats()["hashes"] == n - first
        r = pool.read()
        assert r.status.tolist() == status and r.parent.tolist() == parent
        assert r.depth.tolist() == depth and r.n_bad.tolist() == n_bad and r.best == best and not b["ok"]
        part = pool.read(T - 3, 4)  # a range across the seam
        assert part.depth.tolist() == depth[T - 3:] and part.status.tolist() == status[T - 3:]


# ---- a seeded fuzz ----
@pytest.mark.parametrize("seed,difficulty", pu.FUZZ[:6])
def test_fuzz_in_random_batches(miner, seed, difficulty):
    blocks = pu.random_pool(seed)
    rng = random.Random(seed + 1)
    pool, mirror, infos = feed(miner, batches_of(blocks, tuple(rng.randint(1, 130) for _ in blocks)), difficulty)
    pool.close()
    assert any(i["reranked"] for i in infos) and not mirror.ok and mirror.best is not None


# ---- find ----
def test_find(miner, tree):
    blocks = [pu.copy_block(b) for b in pu.shuffled(tree, 6)[0]]
    vu.flip_hash_digit(blocks, 9)
    twin = pu.copy_block(blocks[4])
    twin.index += 256
    blocks.append(twin)
    pool, mirror, _ = feed(miner, batches_of(blocks, (7,)), pu.D)
    with pool:
        names = [pu.name_of(b) for b in blocks]
        want = [mirror.find(x) for x in names]
        assert pool.find(names) == want and miner.stats()["launches"] == 1
        assert want[9] == POOL_NONE and want[40] == 4 and mirror.status[9] & V_HASH
        assert sorted(w for w in want if w != POOL_NONE) == sorted([k for k in range(40) if k != 9] + [4])
        name = names[0]
        odd = {rule: PREV_RULES[rule][0](name) for rule in sorted(PREV_RULES)}
        odd = {rule: text for rule, text in odd.items() if len(text) == 64}
        assert sorted(odd) == ["another_digest", "non_hex_character", "uppercase_digit"]
        odd["nul_first"] = b"\0" + name[1:]
        odd["space_last"] = name[:63] + b" "
        assert pool.find([name] + list(odd.values()) + [name]) == [0] + [POOL_NONE] * len(odd) + [0]
        assert pool.find([]) == []
    with miner.open_pool(pu.D) as empty:
        assert empty.find(names[:3]) == [POOL_NONE] * 3 and empty.info()["best"] is None


# ---- isolation ----
def test_two_pools_and_other_calls_by_turns(miner, tree):
    """Two pools at different difficulties fed by turns on one context, with
    pow_index_blocks and pow_verify_chain (the tile staging buffer's other
    users) between the adds: both stay exact."""
    a_blocks, _ = pu.shuffled(tree, 21)
    b_blocks = pu.random_pool(101)[:120]
    chain = vu.build_chain(70, 0, seed=5)
    a = b = ma = mb = None
    try:
        for ka, kb in zip(batches_of(a_blocks, (5,)), batches_of(b_blocks, (15,))):
            a, ma, _ = feed(miner, [ka], pu.D, mirror=ma, pool=a)
            pu.check(miner, b_blocks[:33], 3)
            b, mb, _ = feed(miner, [kb], 1, mirror=mb, pool=b)
            assert miner.verify_chain(chain, 0).ok
            compare(a, ma)
            compare(b, mb)
        assert len(ma) == 40 and len(mb) == 120 and ma.ok and not mb.ok
    finally:
        for p in (a, b):
            if p is not None:
                p.close()


# ---- the calls' refusals on a live pool ----
POISON = 0xA5A5A5A5


def last_error(L) -> str:
    return (L.pow_last_error() or b"").decode()


def test_einval_on_a_live_pool_changes_nothing(miner, tree):
    """Null blocks with m > 0, an add past POW_POOL_MAX_BLOCKS (its pointer is
    never read), a read past the size, null names: POW_EINVAL with the first
    fault's message, nothing written, the pool, its info and the context's
    stats as they were, and the next add goes through."""
    L = miner.L
    pool, mirror, _ = feed(miner, [tree[:5]], pu.D)
    with pool:
        stats = miner.stats()
        info = PoolInfo(*[POISON] * 9)
        words = (ctypes.c_uint32 * 4)(*[POISON] * 4)
        never_read = ctypes.cast(ctypes.c_void_p(8), ctypes.POINTER(Block))
        assert L.pow_pool_add(pool.handle, None, 1, ctypes.byref(info)) == POW_EINVAL and "null blocks" in last_error(L)
        assert L.pow_pool_add(pool.handle, None, 1 << 40, ctypes.byref(info)) == POW_EINVAL
        assert "null blocks" in last_error(L)  # the earlier fault of the two
        for m in ((1 << 20) - 4, 1 << 20, 1 << 40):  # one too many, and more
            assert L.pow_pool_add(pool.handle, never_read, m, ctypes.byref(info)) == POW_EINVAL
            assert "pool too large" in last_error(L), last_error(L)
        for first, count in ((3, 3), (6, 0), (0, 1 << 40), (1 << 40, 1)):
            assert L.pow_pool_read(pool.handle, first, count, None, words, words, words) == POW_EINVAL
            assert "past the pool" in last_error(L), last_error(L)
        assert L.pow_pool_find(pool.handle, None, 1, words) == POW_EINVAL and "null" in last_error(L)
        assert L.pow_pool_find(pool.handle, b"0" * 64, 1, None) == POW_EINVAL and "null" in last_error(L)
        assert L.pow_pool_find(pool.handle, b"0" * 64, (1 << 20) + 1, words) == POW_EINVAL
        assert "too many names" in last_error(L)
        assert [getattr(info, n) for n, _ in PoolInfo._fields_] == [POISON] * 9 and list(words) == [POISON] * 4
        assert miner.stats() == stats and pool.info()["size"] == 5
        compare(pool, mirror)
        assert L.pow_pool_read(pool.handle, 5, 0, None, words, words, words) == 0  # the empty range at the end
        feed(miner, [tree[5:9]], pu.D, mirror=mirror, pool=pool)
        assert len(pool) == 9


def test_a_context_bound_to_a_stop_board_refuses_pool_calls(tree):
    with GpuMiner(0) as m, StopBoard(2) as board:
        L = m.L
        pool, mirror, _ = feed(m, [tree[:5]], pu.D)
        with pool:
            m.bind_board(board, 0, 1)
            try:
                info = PoolInfo(*[POISON] * 9)
                words = (ctypes.c_uint32 * 5)(*[POISON] * 5)
                arr = pu.as_array(tree[5:6])
                assert L.pow_pool_add(pool.handle, arr, 1, ctypes.byref(info)) == POW_EINVAL
                assert "pow_pool_add does not run on a context bound to a stop board" in last_error(L)
                assert L.pow_pool_read(pool.handle, 0, 5, None, words, words, words) == POW_EINVAL
                assert "pow_pool_read does not run" in last_error(L)
                assert L.pow_pool_find(pool.handle, pu.name_of(tree[0]), 1, words) == POW_EINVAL
                assert "pow_pool_find does not run" in last_error(L)
                with pytest.raises(PowError) as e:
                    m.open_pool(pu.D)
                assert e.value.code == POW_EINVAL and "pow_pool_open does not run" in str(e.value)
                assert info.size == POISON and list(words) == [POISON] * 5
                assert pool.info()["size"] == 5  # no GPU work: not refused
            finally:
                m.bind_board(None)
            feed(m, [tree[5:9]], pu.D, mirror=mirror, pool=pool)  # unbound: as before


def test_after_a_failed_add_every_call_fails_at_once(tree):
    """The test library's bounded 300 ms stall kernel in front of the add's
    first launch, behind a 30 ms watchdog (tests/test_gpu_parity.py's watchdog
    tests): the add fails with POW_EHIP, and then every call on the pool but
    pow_pool_close does, without touching the GPU."""
    with helpers.hooked_miner(("POW_TEST_STALL_US", "POW_WATCHDOG_MS"), POW_TEST_STALL_US=300000,
                              POW_WATCHDOG_MS=30) as m:
        L = m.L
        pool = m.open_pool(pu.D)  # its reset goes through no launch hook
        info = PoolInfo(*[POISON] * 9)
        words = (ctypes.c_uint32 * 4)(*[POISON] * 4)
        arr = pu.as_array(tree[:3])
        assert L.pow_pool_add(pool.handle, arr, 3, ctypes.byref(info)) == POW_EHIP and "watchdog" in last_error(L)
        for call in (lambda: L.pow_pool_add(pool.handle, arr, 3, ctypes.byref(info)),
                     lambda: L.pow_pool_add(pool.handle, arr, 0, ctypes.byref(info)),
                     lambda: L.pow_pool_read(pool.handle, 0, 0, None, words, words, words),
                     lambda: L.pow_pool_find(pool.handle, pu.name_of(tree[0]), 1, words),
                     lambda: L.pow_pool_get_info(pool.handle, ctypes.byref(info))):
            assert call() == POW_EHIP and "the pool is unusable after a failed call" in last_error(L), last_error(L)
        assert info.size == POISON and list(words) == [POISON] * 4
        with pytest.raises(PowError) as e:
            m.open_pool(pu.D)
        assert e.value.code == POW_EHIP
        pool.close()  # the one call that still works; the context's close waits the stall out


def test_destroy_keeps_a_context_with_open_pools(tree):
    m = GpuMiner(0)
    try:
        pool, mirror, _ = feed(m, [tree[:5]], pu.D)
        m.L.pow_destroy(m.ctx)  # refused: the pool's calls go through this context
        assert "pow_destroy: 1 pools still open" in last_error(m.L)
        feed(m, [tree[5:9]], pu.D, mirror=mirror, pool=pool)  # both still work
        other = m.open_pool(pu.D)
        m.close()  # the miner closes its pools first, then its context
        assert not pool.handle and not other.handle and not m.ctx
        pool.close()  # nothing left to do
    finally:
        m.close()
