"""Batches of chains for the pow_verify_chains tests, on top of verify_util:
built on the CPU with hashlib only, and the expected result of a batch, which
is the host mirror's (block.verify_chains, block.best_chain)."""
import ctypes

from mpi_blockchain_amd._lib import Block
from mpi_blockchain_amd.block import best_chain, verify_chains

import verify_util as vu

D = 4
# Lengths that cut one 200-block chain into pieces: boundaries inside a wave,
# on the wave boundary (64, 128), one block before and after it, chains of one
# block, empty chains anywhere, and no boundary at all.
SPLITS = ([5] * 40, [1] * 64 + [136], [63, 1, 64, 65, 7], [0, 64, 0, 0, 136, 0], [200])


def split(chain, lengths):
    """Consecutive pieces of `chain` as ctypes arrays of their own."""
    out, at = [], 0
    for n in lengths:
        out.append(vu.copy_chain(chain, at, at + n))
        at += n
    assert at <= len(chain)
    return out


def repeating_lengths(total: int, pattern) -> list:
    """`pattern` over and over until the lengths add up to `total` (the last one cut short)."""
    out, left = [], total
    while left:
        for n in pattern:
            out.append(min(n, left))
            left -= out[-1]
            if not left:
                break
    return out


def cut_in_front_of(total: int, positions) -> list:
    """Lengths that cut `total` blocks right in front of every one of
    `positions`: each of them is the first block of a piece (nobody's parent),
    and the block before it the last of one (nobody's child)."""
    cuts = sorted(set(positions) - {0}) + [total]
    return [b - a for a, b in zip([0] + cuts, cuts)]


def concat(chains):
    total = sum(len(c) for c in chains)
    arr = (Block * max(total, 1))()
    at = 0
    for c in chains:
        for b in c:
            ctypes.memmove(ctypes.byref(arr, at * ctypes.sizeof(Block)), ctypes.addressof(b), ctypes.sizeof(Block))
            at += 1
    return arr, total


def neighbours(n_chains: int = 13, length: int = 5, difficulty: int = D):
    """Unrelated valid chains: different seeds and first_index values, so no
    block links to the one behind it in another chain.  13 x 5 = 65 blocks put
    boundaries inside a wave and chain 12 across the wave boundary."""
    return [vu.build_chain(length, difficulty, seed=20 + c, first_index=1000 * ((7 * c) % n_chains) + 3)
            for c in range(n_chains)]


def expected(chains, difficulty: int):
    """(status per chain, first_bad, n_bad, best, ok) from the host mirror."""
    status = verify_chains(chains, difficulty)
    first = [next((i for i, s in enumerate(st) if s), len(st)) for st in status]
    n_bad = [sum(1 for s in st if s) for st in status]
    return status, first, n_bad, best_chain(chains, status), not any(n_bad)
