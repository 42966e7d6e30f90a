"""Shared pieces of the pow_mine_batch tests: the raw C call, the byte view of
blocks and the recorded reference batch (tests/golden/mined_batch.json)."""
import ctypes
import json
import os

from mpi_blockchain_amd._lib import Block
from mpi_blockchain_amd.block import make_block

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BLOCK_BYTES = ctypes.sizeof(Block)
NONE = 0xFFFFFFFFFFFFFFFF  # found_ctr of an unsolved or unreached template
FILL = 0xA5


def raw(blocks) -> bytes:
    """All 552 bytes of every block, padding included."""
    return b"".join(ctypes.string_at(ctypes.addressof(b), BLOCK_BYTES) for b in blocks)


def array(blocks):
    """The blocks as one C array, copied whole."""
    arr = (Block * max(len(blocks), 1))()
    for i, b in enumerate(blocks):
        ctypes.memmove(ctypes.byref(arr, i * BLOCK_BYTES), ctypes.addressof(b), BLOCK_BYTES)
    return arr


def call(L, ctx, tmpls, difficulty, ctr_start, ctr_count, cancel=None, epoch=0, in_place=False):
    """pow_mine_batch as C sees it: (rc, n_solved, hashes, counters, out).
    `out` is a Block array filled with 0xA5 bytes before the call (in_place: the
    template array itself), `counters` the n found_ctr entries, 12345 before it."""
    n = len(tmpls)
    arr = array(tmpls)
    if in_place:
        out = arr
    else:
        out = (Block * max(n, 1))()
        ctypes.memset(out, FILL, ctypes.sizeof(out))
    ctrs = (ctypes.c_uint64 * max(n, 1))(*([12345] * max(n, 1)))
    solved, hashes = ctypes.c_size_t(12345), ctypes.c_uint64(12345)
    rc = L.pow_mine_batch(ctx, arr, n, difficulty, ctr_start, ctr_count, cancel, epoch, out, ctrs, ctypes.byref(solved),
                          ctypes.byref(hashes))
    return rc, solved.value, hashes.value, list(ctrs)[:n], out


def expected_bytes(stated, n_fill=FILL) -> bytes:
    """What `out` holds after a call whose statement is `stated`: the sealed
    block where solved, the fill where not."""
    return b"".join(raw([b]) if b is not None else bytes([n_fill]) * BLOCK_BYTES for b, _ in stated)


def fixture():
    """(parameters, templates, sealed blocks) of mined_batch.json."""
    with open(os.path.join(GOLDEN, "mined_batch.json")) as f:
        v = json.load(f)
    tmpls = [make_block(e["index"], e["node_owner_number"], e["difficulty"], e["created_at"],
                        bytes.fromhex(e["previous_block_hash_hex"])) for e in v["templates"]]
    sealed = [make_block(e["index"], e["node_owner_number"], e["difficulty"], e["created_at"],
                         bytes.fromhex(e["previous_block_hash_hex"]), bytes.fromhex(m["nonce_hex"]),
                         m["block_hash"].encode())
              for e, m in zip(v["templates"], v["mined"])]
    return v, tmpls, sealed


def race_templates(n, difficulty, base=1_700_000_000, index=1, prev=b""):
    """Template i: owner i, created_at base + 13 i + i^2 mod 7."""
    return [make_block(index, i, difficulty, base + 13 * i + (i * i) % 7, prev) for i in range(n)]
