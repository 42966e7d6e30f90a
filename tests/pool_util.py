"""Pools for the pow_index_blocks tests, built on the CPU with hashlib only
(block.mine_chain, block.mine_race and verify_util's seal: no builder here
calls the code under test), what the tests do to them, and check(): one call
against the mirror."""
import ctypes
import random

import numpy as np

from mpi_blockchain_amd._lib import Block
from mpi_blockchain_amd.block import (POOL_NONE, POOL_ROOT, chain_from, field, index_blocks, make_block, mine_chain,
                                      mine_race, set_field, verify_chain)

import verify_util as vu

D = 4  # what every block of tree() has at the least (its parts are mined at 4 to 8)


def as_array(blocks):
    arr = (Block * max(len(blocks), 1))()
    for i, b in enumerate(blocks):
        ctypes.memmove(ctypes.byref(arr, i * ctypes.sizeof(Block)), ctypes.addressof(b), ctypes.sizeof(Block))
    return arr


def copy_block(b: Block) -> Block:
    c = Block()
    ctypes.memmove(ctypes.addressof(c), ctypes.addressof(b), ctypes.sizeof(Block))
    return c


def genesis(seed: int, difficulty: int = 5, index: int = 1) -> Block:
    """A root: an empty previous_block_hash."""
    return vu.build_chain(1, difficulty, seed=seed, first_index=index)[0]


def tree(seed: int = 1):
    """A forked tree of 40 blocks in mining order (a parent in front of its
    children): a trunk of 12 on a root, a branch of 8 from the trunk's fifth
    block mined at d = 8, a race of three rivals over 5 heights from that
    branch's third (d = 4), every rival's loser of the first height, a branch
    of 4 from the trunk's tip, and a second root with a chain of 7."""
    t = 1_700_000_000
    g = genesis(seed)
    trunk = mine_chain(g, 12, 5, owner=1, created_at=[t + k for k in range(12)])[::-1]
    branch = mine_chain(trunk[4], 8, 8, owner=2, created_at=[t + 100 + k for k in range(8)])[::-1]
    race, winners, _ = mine_race(branch[2], 5, 4, owners=(3, 4, 5), created_at=[t + 200 + k for k in range(15)])
    race, winners = race[::-1], winners[::-1]
    losers = []
    for r in range(3):  # the first height's other rivals, each sealed on its own: the forks a race leaves
        if r != winners[0]:
            losers += mine_chain(branch[2], 1, 4, owner=3 + r, created_at=[t + 200 + r])
    top = mine_chain(trunk[11], 4, 6, owner=6, created_at=[t + 300 + k for k in range(4)])[::-1]
    g2 = genesis(seed + 1, index=7)
    other = mine_chain(g2, 7, 5, owner=7, created_at=[t + 400 + k for k in range(7)])[::-1]
    blocks = [g] + trunk + branch + race + losers + top + [g2] + other
    assert len(blocks) == 40
    return blocks


def shuffled(blocks, seed: int):
    """(the blocks in a random order, perm) with result[k] = blocks[perm[k]]."""
    perm = list(range(len(blocks)))
    random.Random(seed).shuffle(perm)
    return [blocks[p] for p in perm], perm


def flat_chain(n: int, difficulty: int, seed: int):
    """A valid chain of n blocks as a pool in mining order (root first)."""
    c = vu.build_chain(n, difficulty, seed=seed)
    return [copy_block(c[n - 1 - k]) for k in range(n)]


def name_of(b: Block) -> bytes:
    """A block's stored text: what a child carries to name it."""
    return field(b, "block_hash")[:64]


def with_prev(b: Block, prev: bytes, difficulty: int = 0) -> Block:
    """A copy of b with previous_block_hash = prev (all 256 bytes given or NUL
    padded), sealed again: previous_block_hash is hashed."""
    c = copy_block(b)
    set_field(c, "previous_block_hash", prev)
    vu.seal(c, difficulty, 12345)
    return c


def sound_tips(pool, difficulty: int):
    """Per block: the chain under it, extracted with chain_from along the
    mirror's parents, has an all-zero verify_chain status and ends at a root."""
    status, parent, depth, n_bad, best = index_blocks(pool, difficulty)
    out = []
    for i in range(len(pool)):
        chain = chain_from(pool, parent, i)
        assert len(chain) == depth[i]
        ends_at_root = field(chain[len(chain) - 1], "previous_block_hash")[0] == 0
        out.append(ends_at_root and not any(verify_chain(chain, difficulty)))
    return out


def launches(n: int) -> int:
    """The plan's: one K10a per host tile, K10b, K10c, ceil(log2 n) rounds of K10d, K10e."""
    return 0 if n == 0 else (n + vu.HOST_TILE - 1) // vu.HOST_TILE + 3 + (n - 1).bit_length()


def check(miner, pool, difficulty, want=None):
    """One call over `pool` against the mirror (`want`: its five results,
    where the caller has them already)."""
    status, parent, depth, n_bad, best = index_blocks(pool, difficulty) if want is None else want
    r = miner.index_blocks(pool, difficulty)
    n = len(pool)
    assert r.status.dtype == np.uint8 and r.status.tolist() == list(status)
    assert r.parent.tolist() == list(parent)
    assert r.depth.tolist() == list(depth)
    assert r.n_bad.tolist() == list(n_bad)
    assert r.best == best
    assert r.ok == (not any(status))
    s = miner.stats()
    assert s["hashes"] == n and s["launches"] == launches(n)
    assert (s["kernel_ms"] > 0) == (n > 0)
    return r


# ---- the fork choice on ties: 600 roots, two workgroups of 256 and one of 88 whose last wave has 24 lanes ----
TIE_N = 600
TIE_CASES = {  # name -> (index by position (9 elsewhere), the flagged positions, best)
    "tie_across_workgroups": ({44: 10, 300: 10}, (), 44),
    "tie_across_waves": ({70: 10, 200: 10}, (), 70),
    "all_equal": ({}, (), 0),
    "flagged_maximum_in_the_ragged_wave": ({577: 0xFFFFFFFF, 599: 0xFFFFFFFE}, (577,), 599),
    "index_0_alone": ({599: 0}, range(599), 599),
    "all_flagged": ({}, range(TIE_N), None),
    "all_ones_leads_a_workgroup": ({256: 0xFFFFFFFF}, (), 256),
}


def tie_pool(case: str):
    """(pool, best) of a TIE_CASES entry: roots sealed at d = 0 with the given
    indices; a flagged one has a digit of its stored text flipped (V_HASH)."""
    index, flagged, best = TIE_CASES[case]
    pool = [genesis(7000 + k, 0, index=index.get(k, 9)) for k in range(TIE_N)]
    for k in flagged:
        vu.flip_hash_digit(pool, k)
    return pool, best


# ---- twins of one digest from every workgroup of K10b ----
def twin_storm(low_index: int, other_index: int):
    """(pool, the positions of C's copies): three unrelated roots, a twin of a
    root R (index 1) at position 3 with `low_index`, then 700 twins of R with
    `other_index` and 100 copies of R's child C (index 2), every eighth block
    a copy of C: 804 blocks, four workgroups of 256.  The indices differ from 1
    in bytes that are not hashed, so all twins have R's digest."""
    r, c = flat_chain(2, 0, seed=41)
    assert (r.index, c.index) == (1, 2) and low_index & 0xFF == other_index & 0xFF == 1
    pool = [genesis(42 + k, 0) for k in range(3)] + [copy_block(r)]
    pool[3].index = low_index
    for k in range(800):
        pool.append(copy_block(c if k % 8 == 7 else r))
        if k % 8 != 7:
            pool[-1].index = other_index
    return pool, [4 + k for k in range(800) if k % 8 == 7]


# ---- every byte at every position of previous_block_hash's 64 characters ----
def name_sweep():
    """(pool, name): a root R, then its child C once per position p of R's name
    and byte v other than the name's, with that one byte replaced (sealed
    again: the field is hashed).  64 x 255 + 1 = 16,321 blocks; the child with
    v = 0 at p = 0 stands at position 1."""
    r, c = flat_chain(2, 0, seed=31)
    name = name_of(r)
    pool = [r]
    for p in range(64):
        pool += [with_prev(c, name[:p] + bytes([v]) + name[p + 1:]) for v in range(256) if v != name[p]]
    return pool, name


# ---- a seeded fuzz ----
# (random_pool's seed, the call's difficulty): V_WORK comes from the blocks' own digests.  Seeds 108 and 109 are
# left out: at d = 3 none of their roots has the work, so no tip is sound (tests/test_pool_host.py asks for one).
FUZZ = [(seed, (0, 1, 3)[k % 3]) for k, seed in enumerate(s for s in range(100, 126) if s not in (108, 109))]


def random_pool(seed: int):
    """A random forest of 200 to 700 blocks sealed at d = 0 (a new block hangs on
    a random earlier one, or is a new root), then about 2 % of the blocks each:
    a flipped digit of the stored text, a flipped nonce, an index off by one, a
    broken previous_block_hash, a duplicate put in at a random position (every
    other one with 256 added to its index, which is not hashed) and a block
    taken out; shuffled."""
    rng = random.Random(seed)
    n = rng.randint(200, 700)
    blocks = []
    for j in range(n):
        if j == 0 or rng.random() < 0.08:
            b = make_block(rng.randrange(1, 40), rng.randrange(8), 0, 1_700_000_000 + j, b"")
        else:
            par = rng.choice(blocks)
            b = make_block(par.index + 1, rng.randrange(8), 0, 1_700_000_000 + j, field(par, "block_hash"))
        vu.seal(b, 0, rng.randrange(62 ** 9 - (1 << 32)))
        blocks.append(b)
    few = max(1, n // 50)
    for tamper in (vu.flip_hash_digit, vu.flip_nonce, vu.index_off_by_one, vu.break_prev):
        for i in rng.sample(range(n), few):
            tamper(blocks, i)
    for k in range(few):
        twin = copy_block(blocks[rng.randrange(len(blocks))])
        twin.index = (twin.index + 256 * (k & 1)) & 0xFFFFFFFF
        blocks.insert(rng.randrange(len(blocks) + 1), twin)
    for _ in range(few):
        del blocks[rng.randrange(len(blocks))]
    rng.shuffle(blocks)
    return blocks


def twins_in(pool, status) -> int:
    """How many named blocks (not V_HASH) share their stored text with an earlier one."""
    names = [name_of(b) for b, s in zip(pool, status) if not s & 1]
    return len(names) - len(set(names))


__all__ = ["D", "POOL_NONE", "POOL_ROOT", "as_array", "copy_block", "genesis", "tree", "shuffled", "flat_chain",
           "name_of", "with_prev", "sound_tips", "launches", "check", "TIE_N", "TIE_CASES", "tie_pool", "twin_storm",
           "name_sweep", "FUZZ", "random_pool", "twins_in"]
