"""pow_index_blocks (K10) where its first tests do not reach: the fork choice
on ties across waves and workgroups and at the ends of the index range (K10e),
hundreds of twins racing for one slot from four workgroups (K10b), every byte
at every position of previous_block_hash's name (K10a's unhex4), the
256-thread seam of K10b to K10e and a seeded fuzz.  Every pool is built with
hashlib at d = 0 (tests/pool_util.py); every call goes through check(), which
compares all five results and the stats with the mirror
(block.index_blocks), and the expectations stated beside it are explicit, so
that a fault shared by mirror and kernel cannot hide.  What these inputs must
hold is pinned without a GPU in tests/test_pool_host.py."""
import pytest

from mpi_blockchain_amd.block import POOL_NONE, POOL_ROOT, V_HASH, V_INDEX, V_LINK, index_blocks
from mpi_blockchain_amd.miner import GpuMiner

import helpers
import pool_util as pu
from pool_util import check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def miner():
    with GpuMiner(0) as m:
        yield m


@pytest.fixture(scope="module")
def smallest_table():
    """POW_POOL_SLOTS_LOG2 at its minimum: the lowest power of two above n."""
    with helpers.hooked_miner(("POW_POOL_SLOTS_LOG2",), POW_POOL_SLOTS_LOG2=1) as m:
        yield m


# ---- a: the fork choice ----
@pytest.mark.parametrize("case", sorted(pu.TIE_CASES))
def test_fork_choice_ties_and_index_range(miner, case):
    """600 roots: the greatest index wins, the lowest position on a tie,
    whichever wave or workgroup holds it; a flagged block never does; a key of
    index 0 counts, and so does one of index 0xFFFFFFFF."""
    pool, best = pu.tie_pool(case)
    index, flagged, _ = pu.TIE_CASES[case]
    r = check(miner, pool, 0)
    assert r.best == best
    assert r.ok == (len(flagged) == 0)
    assert [k for k in range(pu.TIE_N) if r.status[k]] == list(flagged) and set(r.status.tolist()) <= {0, V_HASH}
    assert r.parent.tolist() == [POOL_ROOT] * pu.TIE_N and r.depth.tolist() == [1] * pu.TIE_N
    if best is not None:
        assert pool[best].index == max([index.get(k, 9) for k in range(pu.TIE_N) if k not in flagged])


# ---- b: twins ----
@pytest.mark.parametrize("table", ["shipped", "smallest"])
@pytest.mark.parametrize("low_index, other_index", [(1, 257), (257, 1)])
def test_twin_storm(miner, smallest_table, table, low_index, other_index):
    """701 blocks of one digest from four workgroups: the lowest position keeps
    the name, and its index, which is not hashed, decides its children's
    V_INDEX.  Then the pool reversed: the lowest twin is the one that stood
    last, behind every child."""
    m = miner if table == "shipped" else smallest_table
    pool, children = pu.twin_storm(low_index, other_index)
    n = len(pool)
    assert n == 804 and len(children) == 100 and children[0] == 11 and children[-1] == n - 1
    r = check(m, pool, 0)
    want = 0 if low_index == 1 else V_INDEX
    assert [(int(r.parent[k]), int(r.status[k])) for k in children] == [(3, want)] * 100
    assert [int(r.status[k]) for k in range(n) if k not in children] == [0] * 704
    assert r.best == (4 if low_index == 1 else 3)  # the first of index 257
    back = pool[::-1]
    low = n - 1 - (n - 2)  # the last twin: position n - 2 of the pool, behind it only a copy of C
    assert back[low].index == other_index and back[0].index == 2
    r = check(m, back, 0)
    want = 0 if other_index == 1 else V_INDEX
    assert [(int(r.parent[n - 1 - k]), int(r.status[n - 1 - k])) for k in children] == [(low, want)] * 100
    assert r.best == (low if other_index == 257 else n - 1 - 3)


# ---- c: the parser of previous_block_hash ----
def test_every_byte_at_every_position_of_the_name(miner):
    """One wrong byte anywhere in the 64 characters names nobody: whatever the
    byte's low nibble is, and whichever of the three dwords it stands in.  A
    NUL in front makes a root; a NUL later cuts the name short."""
    pool, name = pu.name_sweep()
    assert len(pool) == 16321 and set(name) == set(b"0123456789abcdef")
    r = check(miner, pool, 0)
    assert miner.stats()["launches"] == 18  # one host tile
    assert r.parent.tolist() == [POOL_ROOT] * 2 + [POOL_NONE] * 16319
    assert r.status.tolist() == [0] * 2 + [V_LINK] * 16319
    # a pool of that shape does link: the untouched child, 64 times
    r = check(miner, pool[:1] + [pu.copy_block(pu.flat_chain(2, 0, seed=31)[1]) for _ in range(64)], 0)
    assert r.ok and r.parent.tolist() == [POOL_ROOT] + [0] * 64 and r.best == 1


# ---- d: the 256-thread seam of K10b to K10e, and a fuzz ----
@pytest.fixture(scope="module")
def chain513():
    return pu.flat_chain(513, 0, seed=61)


@pytest.mark.parametrize("n", [255, 256, 257, 511, 512, 513])
def test_sizes_around_the_workgroup(miner, chain513, n):
    pool, perm = pu.shuffled(chain513[:n], 200 + n)
    r = check(miner, pool, 0)
    assert r.ok and r.best is not None
    assert pool[r.best].index == n and r.depth[r.best] == n and r.n_bad.tolist() == [0] * n
    assert sorted(r.depth.tolist()) == list(range(1, n + 1))
    assert perm[r.best] == n - 1 and [perm[int(p)] if p < n else p for p in r.parent] == [
        q - 1 if q else POOL_ROOT for q in perm]


@pytest.mark.parametrize("seed, difficulty", pu.FUZZ)
def test_random_pools_against_the_mirror(miner, seed, difficulty):
    pool = pu.random_pool(seed)
    want = index_blocks(pool, difficulty)
    assert 0 in want[3] and any(want[0])  # a sound tip and a flagged block: tests/test_pool_host.py pins the rest
    r = check(miner, pool, difficulty, want)
    assert r.best is not None and not r.ok
