"""Shared pieces of the deep-counter tests: the certified stretch
(tests/golden/deep_stretch.json), its hashlib references, the rows of starts
that reach every digit of a relative counter, and the expected bytes.  Nothing
here calls the code under test: every expected value is hashlib's, directly or
through the host statements block.mine_chain, block.mine_batch and
block.mine_race over the 100 counters around the stretch's solution (sealing
does not depend on ctr_start)."""
import functools
import hashlib
import json
import os

from mpi_blockchain_amd.block import field, make_block, mine_batch, mine_chain, mine_race
from oracle.oracle import py_block_to_str, py_nonce_from_counter

import batch_util as bu
import chain_util as cu
import helpers
import race_util as ru

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NEED = 62 ** 5 + 2 ** 20   # the stretch's least length
OWNERS = [5, 261]          # equal in their low byte: the same message, the same digests
AROUND = 50                # the statements run over [counter - AROUND, counter + AROUND)
SLICE = 1 << 22            # the oracle re-sweeps slices of this many counters
SWITCHES = ("POW_CHAIN_BATCH", "POW_CHAIN_FUSED_MAX", "POW_CHAIN_LANES_LOG2", "POW_BATCH_FUSED_MAX", "POW_BATCH_TILE",
            "POW_BATCH_LANES_LOG2", "POW_RACE_FUSED_MAX", "POW_RACE_BATCH", "POW_RACE_LANES_LOG2")
FUSED = {"POW_CHAIN_FUSED_MAX": 32, "POW_BATCH_FUSED_MAX": 32, "POW_RACE_FUSED_MAX": 32}
LOOPS = {"POW_CHAIN_FUSED_MAX": -1, "POW_BATCH_FUSED_MAX": -1, "POW_RACE_FUSED_MAX": -1}


@functools.lru_cache(maxsize=None)
def stretch() -> dict:
    with open(os.path.join(GOLDEN, "deep_stretch.json")) as f:
        return json.load(f)


def parent():
    p = stretch()["parent"]
    return make_block(p["index"], p["node_owner_number"], p["difficulty"], p["created_at"])


def template(owner):
    """pow_mine_chain's refresh of the parent for `owner` (node.cpp:292-299)."""
    s, p = stretch(), parent()
    return make_block(p.index + 1, owner, s["difficulty"], s["created_at"], prev=field(p, "block_hash"),
                      block_hash=field(p, "block_hash"))


def digest_of(ctr: int) -> bytes:
    """hashlib over block_to_str (block.cpp:79-88, restated in Python) of the
    stretch's template with counter `ctr`'s nonce; the owners share it."""
    s = stretch()
    return hashlib.sha256(py_block_to_str(s["parent"]["index"] + 1, s["owner"], s["difficulty"], s["created_at"],
                                          py_nonce_from_counter(ctr), bytes(256))).digest()


def lz_of(digest: bytes) -> int:
    return 256 - int.from_bytes(digest, "big").bit_length()


def sealed(owner) -> bytes:
    """All 552 bytes of `owner`'s template sealed with the stretch's solution, by hashlib alone."""
    t = cu.raw([template(owner)])
    ctr = stretch()["counter"]
    # nonce[10] at byte 24, block_hash at 290: the hex and its NUL over the first 65 bytes (node.cpp:318)
    return t[:24] + py_nonce_from_counter(ctr) + t[34:290] + digest_of(ctr).hex().encode() + b"\0" + t[355:]


def window_around():
    return stretch()["counter"] - AROUND, 2 * AROUND


@functools.lru_cache(maxsize=None)
def stated_chain() -> bytes:
    s = stretch()
    chain = mine_chain(parent(), 1, s["difficulty"], s["owner"], [s["created_at"]], *window_around())
    assert len(chain) == 1
    return cu.raw(chain)


@functools.lru_cache(maxsize=None)
def stated_batch():
    """(bytes of both sealed templates, counters)."""
    stated = mine_batch([template(o) for o in OWNERS], stretch()["difficulty"], *window_around())
    assert all(b is not None for b, _ in stated)
    return bu.expected_bytes(stated), [c for _, c in stated]


@functools.lru_cache(maxsize=None)
def stated_race(owners: tuple):
    """(bytes, winners, counters) of a race of `owners` with equal created_at."""
    s = stretch()
    blocks, winners, counters = mine_race(parent(), 1, s["difficulty"], list(owners), [s["created_at"]] * len(owners),
                                          *window_around())
    assert len(blocks) == 1
    return ru.raw(blocks), winners, counters


def rows() -> dict:
    """name -> (ctr_start, ctr_count, solves): what each start reaches is in the
    test module's docstring.  Where nothing else is said the window ends 1,000
    counters past the solution."""
    s = stretch()
    a, b = s["empty_from"], s["counter"]
    out = {"far": (a, b - a + 1000, True),                       # every digit of rel
           "max_window": (a, 1 << 32, True),                     # L.count = 2^32
           "one": (b - 62 ** 5, 62 ** 5 + 1000, True),           # rel's digits 1,0,0,0,0,0
           "nines": (b - (62 ** 5 - 1), 62 ** 5 + 999, True),    # five digits of 61
           "step3": (b - 62 ** 3, 62 ** 3 + 1000, True),
           "step4": (b - 62 ** 4, 62 ** 4 + 1000, True),
           "key_over": (b - 2 ** 24, 2 ** 24 + 1000, True),      # K6's key needs 33 bits
           "key_under": (b - (2 ** 24 - 1), 2 ** 24 + 999, True),  # ... and 32
           "edge_last": (b - 2 ** 24, 2 ** 24 + 1, True),        # solves on the window's last counter
           "edge_none": (b - 2 ** 24, 2 ** 24, False)}           # ends at the solution, exclusive
    for start, count, _ in out.values():
        assert a <= start and start + count <= 62 ** 9 and 1 <= count <= 1 << 32
    return out


ROW_NAMES = ("far", "max_window", "one", "nines", "step3", "step4", "key_over", "key_under", "edge_last", "edge_none")
SWAPPED_ROWS = ("step3", "step4", "key_over", "key_under")  # the race with owners [261, 5] too


def miner_with(**switches):
    """A context of the test library whose pow_init saw exactly these switches."""
    return helpers.hooked_miner(SWITCHES, **switches)
