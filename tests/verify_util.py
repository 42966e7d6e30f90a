"""Chains for the pow_verify_chain tests, built on the CPU with hashlib only
(nothing here calls the code under test), tip first as on the wire."""
import ctypes
import hashlib
import json
import os
import random

from mpi_blockchain_amd._lib import Block
from mpi_blockchain_amd.block import field, make_block, set_field, verify_chain
from oracle.oracle import py_block_to_str, py_nonce_from_counter

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HOST_TILE = 1 << 16  # pow_verify_chain's host tile: block HOST_TILE is the first tile's halo


def message(b: Block) -> bytes:
    """block_to_str (block.cpp:79-88), restated in Python."""
    return py_block_to_str(b.index, b.node_owner_number, b.difficulty, b.created_at, field(b, "nonce"),
                           field(b, "previous_block_hash"))


def leading_zero_bits(b: Block) -> int:
    return 256 - int.from_bytes(hashlib.sha256(message(b)).digest(), "big").bit_length()


def seal(b: Block, difficulty: int, ctr: int) -> None:
    """Nonces from counter `ctr` up until the block's digest has `difficulty`
    leading zero bits; block_hash = its hex (strcpy: later bytes stay)."""
    while True:
        set_field(b, "nonce", py_nonce_from_counter(ctr))
        digest = hashlib.sha256(message(b)).digest()
        if 256 - int.from_bytes(digest, "big").bit_length() >= difficulty:
            break
        ctr += 1
    ctypes.memmove(ctypes.addressof(b) + Block.block_hash.offset, digest.hex().encode() + b"\0", 65)


def build_chain(n: int, difficulty: int, seed: int = 1, first_index: int = 1):
    """A valid chain of n blocks as a ctypes array, tip first.  The oldest
    block has an empty previous_block_hash; every other one the 256 bytes of
    its parent's block_hash (the memcpy of node.cpp:299)."""
    rng = random.Random(seed)
    arr = (Block * n)()
    prev = b""
    for j in range(n):
        b = make_block(first_index + j, rng.randrange(8), difficulty, 1_700_000_000 + 7 * j, prev)
        seal(b, difficulty, rng.randrange(62 ** 9 - (1 << 32)))
        arr[n - 1 - j] = b
        prev = field(b, "block_hash")
    return arr


def copy_chain(arr, lo: int = 0, hi: int | None = None):
    hi = len(arr) if hi is None else hi
    out = (Block * (hi - lo))()
    if hi > lo:
        ctypes.memmove(out, ctypes.byref(arr, lo * ctypes.sizeof(Block)), (hi - lo) * ctypes.sizeof(Block))
    return out


# ---- corruptions: each takes the chain and a position and changes one block in place ----
def flip_nonce(c, i):
    raw = bytearray(field(c[i], "nonce"))
    raw[3] = ord("b") if raw[3] == ord("a") else ord("a")
    set_field(c[i], "nonce", bytes(raw))


def flip_hash_digit(c, i):
    raw = bytearray(field(c[i], "block_hash"))
    raw[17] = ord("1") if raw[17] == ord("0") else ord("0")
    set_field(c[i], "block_hash", bytes(raw))


def unterminated_hash(c, i):
    raw = bytearray(field(c[i], "block_hash"))
    raw[64] = ord("x")
    set_field(c[i], "block_hash", bytes(raw))


def break_prev(c, i):
    raw = bytearray(field(c[i], "previous_block_hash"))
    raw[40] = ord("f") if raw[40] != ord("f") else ord("e")
    set_field(c[i], "previous_block_hash", bytes(raw))


def index_off_by_one(c, i):
    c[i].index = (c[i].index + 1) & 0xFFFFFFFF


def index_wrap(c, i):
    """Index 0 over a parent of index 0xFFFFFFFF: consecutive in uint32_t."""
    c[i].index = 0
    if i + 1 < len(c):
        c[i + 1].index = 0xFFFFFFFF


CORRUPTIONS = {"nonce": flip_nonce, "hash_digit": flip_hash_digit, "unterminated_hash": unterminated_hash,
               "prev": break_prev, "index": index_off_by_one, "index_wrap": index_wrap}


def mirror(chain, difficulty: int) -> list:
    return verify_chain(chain, difficulty)


def expected_after(base_status, chain, touched, difficulty: int) -> list:
    """The mirror's status of `chain`, which differs from a chain of status
    `base_status` only in the blocks `touched`: a block's status depends on
    itself and its parent, so only the touched blocks and their children are
    evaluated again (the mirror over 65,538 blocks takes two seconds)."""
    n = len(chain)
    want = list(base_status)
    for i in sorted({j for t in touched for j in (t - 1, t) if 0 <= j < n}):
        want[i] = verify_chain(copy_chain(chain, i, min(n, i + 2)), difficulty)[0]
    return want


def fixture_chain():
    """tests/golden/chain_vectors.json as (ctypes array tip first, difficulty)."""
    with open(os.path.join(GOLDEN, "chain_vectors.json")) as f:
        v = json.load(f)
    arr = (Block * len(v["chain"]))()
    for i, e in enumerate(v["chain"]):
        b = make_block(e["index"], e["node_owner_number"], e["difficulty"], e["created_at"],
                       bytes.fromhex(e["previous_block_hash_hex"]), bytes.fromhex(e["nonce_hex"]),
                       e["block_hash"].encode())
        arr[i] = b
    return arr, v["difficulty"]
