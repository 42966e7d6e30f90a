"""Shared pieces of the pow_mine_race tests: the raw C call, the byte view of
blocks and the recorded reference races (tests/golden/mined_race.json)."""
import ctypes
import json
import os

from mpi_blockchain_amd._lib import Block
from mpi_blockchain_amd.block import make_block

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BLOCK_BYTES = ctypes.sizeof(Block)
FILL = 0xA5
UNSET_WINNER, UNSET_CTR = 0xA5A5A5A5, 12345  # winners / found_ctr entries the call did not write


def raw(blocks) -> bytes:
    """All 552 bytes of every block, padding included."""
    return b"".join(ctypes.string_at(ctypes.addressof(b), BLOCK_BYTES) for b in blocks)


def call(L, ctx, parent, n, difficulty, owners, created_at, ctr_start, ctr_count, cancel=None, epoch=0,
         n_rivals=None):
    """pow_mine_race as C sees it: (rc, n_mined, hashes, winners, counters, out).
    `out` is a Block * n array filled with 0xA5 bytes before the call; `winners`
    and `counters` are the n entries, UNSET_WINNER and UNSET_CTR before it."""
    R = len(owners) if n_rivals is None else n_rivals
    own = (ctypes.c_uint32 * max(len(owners), 1))(*owners)
    out = (Block * max(n, 1))()
    ctypes.memset(out, FILL, ctypes.sizeof(out))
    times = (ctypes.c_uint64 * max(len(created_at), 1))(*created_at) if created_at is not None else None
    win = (ctypes.c_uint32 * max(n, 1))(*([UNSET_WINNER] * max(n, 1)))
    ctrs = (ctypes.c_uint64 * max(n, 1))(*([UNSET_CTR] * max(n, 1)))
    mined, hashes = ctypes.c_size_t(12345), ctypes.c_uint64(12345)
    rc = L.pow_mine_race(ctx, ctypes.byref(parent) if parent is not None else None, n, difficulty, own, R, times,
                         ctr_start, ctr_count, cancel, epoch, out, win, ctrs, ctypes.byref(mined), ctypes.byref(hashes))
    return rc, mined.value, hashes.value, list(win)[:n], list(ctrs)[:n], out


def expected(stated, n):
    """(bytes of out, winners, counters) after a call over n heights whose
    statement is `stated` = (blocks, winners, counters), tip first: the mined
    heights at the upper end, the fill below them."""
    blocks, winners, counters = stated
    k = n - len(blocks)
    return (bytes([FILL]) * (k * BLOCK_BYTES) + raw(blocks), [UNSET_WINNER] * k + list(winners),
            [UNSET_CTR] * k + list(counters))


def _block(e: dict) -> Block:
    return make_block(e["index"], e["node_owner_number"], e["difficulty"], e["created_at"],
                      bytes.fromhex(e["previous_block_hash_hex"]), bytes.fromhex(e["nonce_hex"]),
                      bytes.fromhex(e["block_hash_hex"]))


def fixture():
    """(parameters, parent, {name: (race, chain tip first)}) of mined_race.json."""
    with open(os.path.join(GOLDEN, "mined_race.json")) as f:
        v = json.load(f)
    return v, _block(v["parent"]), {name: (r, [_block(e) for e in r["chain"]]) for name, r in v["races"].items()}


def times(n, R, base=1_700_000_000):
    """created_at distinct per (height, rival), height-major."""
    return [base + 17 * k + 5 * r + (k * r) % 3 for k in range(n) for r in range(R)]


def genesis() -> Block:
    """initialize_first_block (node.cpp:361-372): index 0, block_hash zeroed."""
    return make_block(0, 0, 9, 1_699_999_990)
