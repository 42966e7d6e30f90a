"""Pools for the pow_index_blocks tests, built on the CPU with hashlib only
(block.mine_chain, block.mine_race and verify_util's seal: nothing here calls
the code under test), and what the tests do to them."""
import ctypes
import random

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


__all__ = ["D", "POOL_NONE", "POOL_ROOT", "as_array", "copy_block", "genesis", "tree", "shuffled", "flat_chain",
           "name_of", "with_prev", "sound_tips"]
