"""Shared pieces of the pow_mine_chain tests: the raw C call, the byte view of
a chain and the recorded reference chain (tests/golden/mined_chain.json)."""
import ctypes
import json
import os

from mpi_blockchain_amd._lib import Block
from mpi_blockchain_amd.block import make_block

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BLOCK_BYTES = ctypes.sizeof(Block)


def genesis() -> Block:
    """initialize_first_block (node.cpp:361-372): index 0, block_hash zeroed."""
    return make_block(0, 0, 9, 1_699_999_990)


def raw(blocks) -> bytes:
    """All 552 bytes of every block, padding included."""
    return b"".join(ctypes.string_at(ctypes.addressof(b), BLOCK_BYTES) for b in blocks)


def call(L, ctx, parent, n, difficulty, owner, created_at, ctr_start, ctr_count, cancel=None, epoch=0, fill=0xA5):
    """pow_mine_chain as C sees it: (rc, n_mined, hashes, out), `out` a Block * n
    array filled with `fill` bytes before the call."""
    out = (Block * max(n, 1))()
    ctypes.memset(out, fill, ctypes.sizeof(out))
    times = (ctypes.c_uint64 * max(n, 1))(*created_at) if created_at is not None else None
    mined, hashes = ctypes.c_size_t(12345), ctypes.c_uint64(12345)
    rc = L.pow_mine_chain(ctx, ctypes.byref(parent) if parent is not None else None, n, difficulty, owner, times,
                          ctr_start, ctr_count, cancel, epoch, out, ctypes.byref(mined), ctypes.byref(hashes))
    return rc, mined.value, hashes.value, out


def _block(e: dict) -> Block:
    return make_block(e["index"], e["node_owner_number"], e["difficulty"], e["created_at"],
                      bytes.fromhex(e["previous_block_hash_hex"]), bytes.fromhex(e["nonce_hex"]),
                      bytes.fromhex(e["block_hash_hex"]))


def fixture():
    """(parameters, parent, chain tip first) of mined_chain.json."""
    with open(os.path.join(GOLDEN, "mined_chain.json")) as f:
        v = json.load(f)
    return v, _block(v["parent"]), [_block(e) for e in v["chain"]]
