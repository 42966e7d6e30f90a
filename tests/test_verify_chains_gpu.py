"""pow_verify_chains on the GPU against its host statements
(mpi_blockchain_amd.block.verify_chains and best_chain).  The chains are built
on the CPU with hashlib at d = 4, plus one of 65,538 blocks at d = 0, so no
input depends on the code under test; every expected value is the mirror's.
K3's link and hex edge matrices (tests/verify_edges.py) go through the
segmentation too, and the long chain once more as 98,307 chains, half of them
empty, across both host tiles."""
import bisect
import ctypes

import numpy as np
import pytest

from mpi_blockchain_amd._lib import Block, PowStats
from mpi_blockchain_amd.block import V_HASH, V_INDEX, V_LINK, V_WORK, make_block
from mpi_blockchain_amd.miner import GpuMiner

import verify_chains_util as cu
import verify_edges as ve
import verify_util as vu

pytestmark = pytest.mark.gpu

D = cu.D
T = vu.HOST_TILE
BIG = T + 2  # 65,538: two host tiles, one halo block across their seam


@pytest.fixture(scope="module")
def miner():
    with GpuMiner(0) as m:
        yield m


@pytest.fixture(scope="module")
def chain200():
    return vu.build_chain(200, D, seed=5)


@pytest.fixture(scope="module")
def thirteen():
    return cu.neighbours()


@pytest.fixture(scope="module")
def big_chain():
    """65,538 blocks at difficulty 0: no mining needed.  Valid, so every slice
    of it is valid (a slice's last block only loses checks)."""
    c = vu.build_chain(BIG, 0, seed=6)
    assert not any(vu.mirror(c, 0))
    return c


def check(miner, chains, difficulty, want=None):
    """One call over `chains` against the mirror (`want`: its status per
    chain, where the caller has it already)."""
    status, first, n_bad, best, ok = cu.expected(chains, difficulty) if want is None else want
    r = miner.verify_chains(chains, difficulty)
    assert len(r.status) == len(chains)
    for c, st in enumerate(r.status):
        assert st.dtype == np.uint8 and st.tolist() == list(status[c]), c
    assert r.first_bad == first
    assert r.n_bad == n_bad
    assert r.best == best
    assert r.ok == ok
    total = sum(len(c) for c in chains)
    s = miner.stats()
    assert s["hashes"] == total and s["launches"] == (total + T - 1) // T
    assert (s["kernel_ms"] > 0) == (total > 0)
    return r


def clean(chains, best):
    """The expected result of valid chains whose mirror the caller has."""
    return [[0] * len(c) for c in chains], [len(c) for c in chains], [0] * len(chains), best, True


def test_unrelated_neighbours(miner, thirteen):
    r = check(miner, thirteen, D)
    assert r.ok and r.n_bad == [0] * 13 and r.first_bad == [5] * 13
    assert r.best == max(range(13), key=lambda c: thirteen[c][0].index)
    # not vacuous: the same buffer as ONE chain has a broken link and index at every boundary
    arr, total = cu.concat(thirteen)
    one = miner.verify_chain(arr, D)
    assert total == 65 and one.n_bad == 12
    assert all(one.status[5 * c + 4] == V_LINK | V_INDEX for c in range(12))


@pytest.mark.parametrize("lengths", cu.SPLITS, ids=lambda s: f"{len(s)}pieces")
def test_pieces_of_one_valid_chain(miner, chain200, lengths):
    pieces = cu.split(chain200, lengths)
    r = check(miner, pieces, D)
    assert r.ok and r.first_bad == list(lengths)
    if list(lengths) == [200]:
        one = miner.verify_chain(chain200, D)
        assert r.status[0].tolist() == one.status.tolist() and (r.first_bad[0], r.n_bad[0]) == (one.first_bad, one.n_bad)


def test_boundaries_cut_the_link(miner, chain200):
    lengths = cu.SPLITS[2]  # [63, 1, 64, 65, 7]
    for k in range(len(lengths) - 1):
        whole = vu.copy_chain(chain200)
        tip = sum(lengths[:k + 1])
        vu.flip_hash_digit(whole, tip)
        assert vu.mirror(vu.copy_chain(whole, tip - 1, tip + 1), D)[0] == V_LINK  # as one chain: a broken link
        r = check(miner, cu.split(whole, lengths), D)
        flagged = [(c, i, int(s)) for c, st in enumerate(r.status) for i, s in enumerate(st) if s]
        assert flagged == [(k + 1, 0, V_HASH)]  # the last block of piece k stays clean


def test_segmented_results(miner, thirteen):
    chains = [vu.copy_chain(c) for c in thirteen]
    top = max(range(13), key=lambda c: chains[c][0].index)
    vu.flip_nonce(chains[0], 0)
    vu.break_prev(chains[6], 2)
    vu.flip_hash_digit(chains[12], 1)     # two in one chain: flags 0 (link), 1 (hash) ...
    vu.index_off_by_one(chains[12], 4)    # ... 3, whose parent's index moved, and 4 (the index is hashed)
    vu.unterminated_hash(chains[top], 3)  # the highest tip is not a valid chain
    r = check(miner, chains, D)
    touched = {0, 6, 12, top}
    for c in range(13):
        if c not in touched:
            assert (r.first_bad[c], r.n_bad[c]) == (5, 0)
    assert r.first_bad[0] == 0 and r.first_bad[6] == 2 and r.first_bad[12] == 0 and r.n_bad[12] == 4
    assert not r.ok and r.best not in touched
    assert r.best == max((c for c in range(13) if c not in touched), key=lambda c: chains[c][0].index)


def test_empty_chains_and_single_blocks(miner, chain200):
    pieces = cu.split(chain200, [0, 0, 5, 0, 1, 0])
    r = check(miner, pieces, D)
    assert r.first_bad == [0, 0, 5, 0, 1, 0] and r.best == 2  # piece 2 holds the chain's tip
    r = check(miner, [], D)
    assert r.ok and r.best is None and r.status == []
    r = check(miner, [[], [], []], D)
    assert r.ok and r.best is None and r.first_bad == [0, 0, 0]
    ones = cu.split(chain200, [1] * 70)  # chains of one block: nobody has a parent
    r = check(miner, ones, D)
    assert r.best == 0
    bad = [vu.copy_chain(c) for c in ones]
    vu.flip_nonce(bad[69], 0)
    r = check(miner, bad, D)
    assert r.n_bad == [0] * 69 + [1] and r.best == 0


def test_nullable_outputs_and_buffer_reuse(miner, thirteen):
    chains = [vu.copy_chain(c) for c in thirteen]
    vu.flip_hash_digit(chains[3], 4)
    vu.break_prev(chains[9], 0)
    full = check(miner, chains, D)
    arr, total = cu.concat(chains)
    L, n = miner.L, len(chains)
    lengths = (ctypes.c_uint32 * n)(*[5] * n)

    def call(status=False, first=False, bad=False, best=False):
        st = np.full(total, 0xEE, dtype=np.uint8)
        f, b, w = (ctypes.c_uint32 * n)(), (ctypes.c_uint32 * n)(), ctypes.c_size_t(77)
        rc = L.pow_verify_chains(miner.ctx, arr, lengths, n, D, st.ctypes.data_as(ctypes.c_void_p) if status else None,
                                 f if first else None, b if bad else None, ctypes.byref(w) if best else None)
        assert rc == 0
        if status:
            assert st.tolist() == np.concatenate(full.status).tolist()
        if first:
            assert list(f) == full.first_bad
        if bad:
            assert list(b) == full.n_bad
        if best:
            assert w.value == full.best

    for alone in range(4):
        call(*[i != alone for i in range(4)])  # each output NULL alone
        call(*[i == alone for i in range(4)])  # each output alone
    call()                                     # all NULL: the return value is the verdict
    call(True, True, True, True)
    # a smaller call after a larger one, through the same device buffers
    check(miner, chains[8:11], D)
    s = PowStats()
    assert L.pow_get_stats(miner.ctx, ctypes.byref(s)) == 0
    assert s.hashes == 15 and s.launches == 1 and s.kernel_ms > 0
    check(miner, thirteen[:2], D)
    # bad arguments on a live context, and the empty calls
    w = ctypes.c_size_t(77)
    assert L.pow_verify_chains(miner.ctx, arr, lengths, n, 257, None, None, None, ctypes.byref(w)) == -1
    assert L.pow_verify_chains(miner.ctx, None, lengths, n, D, None, None, None, ctypes.byref(w)) == -1
    assert L.pow_verify_chains(miner.ctx, arr, None, n, D, None, None, None, ctypes.byref(w)) == -1
    assert w.value == 77
    assert L.pow_verify_chains(miner.ctx, None, None, 0, D, None, None, None, ctypes.byref(w)) == 1
    assert w.value == ctypes.c_size_t(-1).value


def test_work_boundary(miner, thirteen):
    z = [vu.leading_zero_bits(b) for c in thirteen for b in c]
    zmin = min(z)
    assert zmin >= D
    assert check(miner, thirteen, zmin).ok
    r = check(miner, thirteen, zmin + 1)
    flat = np.concatenate(r.status)
    assert set(flat.tolist()) == {0, V_WORK} and flat[z.index(zmin)] == V_WORK
    for d in (33, 256):  # the full-width path: no 4-bit-mined block has 33 zero bits
        r = check(miner, thirteen, d)
        assert r.n_bad == [5] * 13 and r.best is None
    assert check(miner, thirteen, 0).ok


def test_host_tile_seam_boundary_on_it(miner, big_chain):
    """Global block 65,535 is a chain's last block; its halo, the first block
    of the second tile, is a stranger's tip."""
    first = vu.copy_chain(big_chain, 0, T)
    stranger = vu.build_chain(2, 0, seed=77, first_index=5)
    assert not any(vu.mirror(stranger, 0))
    assert vu.mirror([first[T - 1], stranger[0]], 0)[0] == V_LINK | V_INDEX  # as one chain the seam would flag
    chains = [first, stranger]
    r = check(miner, chains, 0, clean(chains, 0))  # `first` is a slice of a chain whose mirror is all zero
    assert miner.stats()["launches"] == 2 and r.best == 0


def test_host_tile_seam_chain_across_it(miner, big_chain):
    lengths = [T - 6, 8]
    lo = T - 6
    keep = vu.copy_chain(big_chain, lo, BIG)
    vu.flip_hash_digit(big_chain, T)    # flags T itself, and T - 1's link through the seam's halo
    vu.flip_nonce(big_chain, T - 3)
    try:
        chains = cu.split(big_chain, lengths)
    finally:
        ctypes.memmove(ctypes.byref(big_chain, lo * ctypes.sizeof(Block)), keep, ctypes.sizeof(keep))
    tail = vu.mirror(chains[1], 0)
    assert tail == [0, 0, 0, V_HASH, 0, V_LINK, V_HASH, 0]  # both sides of the seam: local 5 is global 65,535
    want = ([[0] * lo, tail], [lo, 3], [0, 3], 0, False)    # chain 0 is a slice of a valid chain
    r = check(miner, chains, 0, want)
    assert r.first_bad[1] == 3 and r.n_bad[1] == 3 and miner.stats()["launches"] == 2


def test_produced_chains(miner):
    """What pow_mine_chain and pow_mine_race produce, audited in one call."""
    parents = [vu.build_chain(1, 9, seed=40 + k, first_index=i)[0] for k, i in enumerate((10, 50, 30, 20))]
    chains = []
    for k in range(3):
        m = miner.mine_chain(parents[k], 4, 9, owner=k, created_at=[1_700_000_100 + j for j in range(4)],
                             ctr_count=1 << 24)
        assert m.complete and m.n_mined == 4
        chains.append(m.blocks)
    race = miner.mine_race(parents[3], 3, 9, owners=(1, 2, 3), created_at=[1_700_000_200 + j for j in range(9)],
                           ctr_count=1 << 24)
    assert race.complete and race.n_mined == 3
    chains.append(race.blocks)
    assert [c[0].index for c in chains] == [14, 54, 34, 23]
    r = check(miner, chains, 9)
    assert r.ok and r.best == 1
    assert check(miner, chains[2:] + chains[:1], 9).best == 0


# ---- K3's edge matrices (tests/verify_edges.py) through the segmentation ----
@pytest.mark.parametrize("lead", [0, 1], ids=["pairs", "behind_one_block"])
def test_link_matrix_as_chains_of_two(miner, lead):
    """Case k's child and parent as a chain of their own.  In the flat chain
    every parent is followed by a stranger, the next case's child, and K3
    rightly flags it; here it is its chain's last block.  Without a leading
    block the parents sit on odd lanes, lane 63 with the stranger in the halo;
    behind one the children do, every 32nd on lane 63 with its parent there."""
    cases = ve.link_cases()
    flat = ve.link_chain(cases)
    n = len(cases)
    chains = ([vu.build_chain(1, 0, seed=91, first_index=77)] if lead else []) + cu.split(flat, [2] * n)
    assert sum(len(c) for c in chains) > 20 * 64
    assert (2 * 31 + 1) % 64 == 63  # case 31's parent without the leading block, its child behind it
    r = check(miner, chains, 0)
    for k, (pc, pp, kind, a, b) in enumerate(cases):
        child, parent = (int(s) for s in r.status[lead + k])
        assert not parent & (V_LINK | V_INDEX), (k, parent)  # a chain's last block has no parent
        assert bool(child & V_LINK) == ve.link_differs(a, b), (pc, pp, kind)
        assert not child & V_INDEX
    # not vacuous: as ONE chain the parents are flagged, each against the next case's child
    one = miner.verify_chain(flat, 0)
    assert all(one.status[2 * k + 1] & V_INDEX for k in range(n - 1))
    assert sum(bool(one.status[2 * k + 1] & V_LINK) for k in range(n - 1)) >= n - 8


def test_hex_matrix_in_pieces(miner):
    """Every text position of block_hash replaced by a NUL in a block of its
    own, and the 400 blocks cut right in front of each of them: V_HASH on the
    corrupted block and nothing else anywhere, since the block in front of it,
    whose link to it is now broken, is the last of its chain."""
    clean_chain = ve.hex_chain()
    bad, used = ve.corrupt_hex(clean_chain, "nul")
    assert len(used) == 64 and sum(V_LINK == s & V_LINK for s in vu.mirror(bad, 0)) == 63  # as one chain: broken links
    lengths = cu.cut_in_front_of(ve.HEX_BLOCKS, used)
    assert sum(lengths) == ve.HEX_BLOCKS and len(lengths) == 64 and 2 in lengths and max(lengths) > 64
    r = check(miner, cu.split(clean_chain, lengths), 0)
    assert r.ok and r.first_bad == lengths
    r = check(miner, cu.split(bad, lengths), 0)
    flagged = [(c, i, int(s)) for c, st in enumerate(r.status) for i, s in enumerate(st) if s]
    assert flagged == [(c, 0, V_HASH) for c in range(0 if 0 in used else 1, 64)]
    # ... and with every piece cut once more in its middle, which cuts no corrupted block from its child
    halves = [h for n in lengths for h in (n - n // 2, n // 2)]
    r = check(miner, cu.split(bad, halves), 0)
    assert sum(r.n_bad) == 64 and all(set(st.tolist()) <= {0, V_HASH} for st in r.status)


# ---- many chains ----
def test_many_chains_across_the_host_tile(miner, big_chain):
    """65,538 blocks as 98,307 chains of 1, 0, 2, 0, 1, 0, ... blocks: a binary
    search 17 steps deep over offsets of which every other one repeats, in both
    launches (the second with base = 65,536)."""
    lengths = cu.repeating_lengths(BIG, (1, 0, 2, 0, 1, 0))
    chains = cu.split(big_chain, lengths)
    n = len(chains)
    assert n > 98000 and lengths.count(0) > 49000 and sum(lengths) == BIG
    starts = np.cumsum([0] + lengths).tolist()
    # the chain of a global position: the last one that starts at or in front of it (the empty ones in front of it too)
    where = {g: bisect.bisect_right(starts, g) - 1 for g in (0, T - 3, T - 1, T, BIG - 1)}
    assert all(starts[c] <= g < starts[c] + lengths[c] for g, c in where.items())
    assert where[0] == 0 and where[T - 1] != where[T] and not any(lengths[where[BIG - 1] + 1:])
    zeros = [[0] * k for k in lengths]  # slices of a valid chain
    check(miner, chains, 0, (zeros, list(lengths), [0] * n, 0, True))
    assert miner.stats()["launches"] == 2 and miner.stats()["hashes"] == BIG
    pair = where[T - 3]
    assert lengths[pair] == 2 and starts[pair] == T - 3  # the last chain of two in front of the seam
    for corrupt, c, i, stated in ((vu.flip_nonce, where[0], 0, [V_HASH]), (vu.flip_hash_digit, where[BIG - 1], 0, [V_HASH]),
                                  (vu.flip_nonce, where[T - 1], 0, [V_HASH]), (vu.flip_hash_digit, where[T], 0, [V_HASH]),
                                  (vu.flip_hash_digit, pair, 1, [V_LINK, V_HASH])):
        keep = vu.copy_chain(chains[c])
        corrupt(chains[c], i)
        try:
            st = vu.mirror(chains[c], 0)
            assert st == stated
            status = zeros[:c] + [st] + zeros[c + 1:]
            first = list(lengths)
            first[c] = next(k for k, s in enumerate(st) if s)
            n_bad = [0] * n
            n_bad[c] = sum(1 for s in st if s)
            best = cu.best_chain(chains, status)
            assert best == (0 if c else 2)  # the highest tip that is left
            check(miner, chains, 0, (status, first, n_bad, best, False))
            assert miner.stats()["launches"] == 2 and miner.stats()["hashes"] == BIG
        finally:
            ctypes.memmove(chains[c], keep, ctypes.sizeof(keep))
