"""Chains for the edge tests of pow_verify_chain's C-string link compare and
hex compare, built on the CPU (random and hashlib; nothing here calls the code
under test).  tests/test_verify_edges_host.py asserts what the constructions
promise; tests/test_verify_edges_gpu.py runs them through the kernel."""
import ctypes
import random

from mpi_blockchain_amd._lib import Block
from mpi_blockchain_amd.block import field, make_block, set_field

import verify_util as vu

# ---- the link matrix ----
NUL_AT = (None, 0, 1, 2, 3, 4, 5, 61, 62, 63, 64, 65, 66, 252, 253, 254, 255)
DIFF_AT = ("none", "byte0", "byte1", "before_nul", "after_nul", "byte254", "byte255")


def _diff_position(kind, pc, pp):
    """Where the one differing byte goes, or None if the combination cannot be
    built: no NUL to be relative to, a position outside the field, or one that
    holds a NUL of either field (the difference must not move a NUL)."""
    nuls = [p for p in (pc, pp) if p is not None]
    first = min(nuls) if nuls else None
    pos = {"byte0": 0, "byte1": 1, "byte254": 254, "byte255": 255,
           "before_nul": None if first is None else first - 1,
           "after_nul": None if first is None else first + 1}[kind]
    if pos is None or not 0 <= pos <= 255 or pos in nuls:
        return None
    return pos


def link_cases(seed: int = 7):
    """(pc, pp, kind, child's previous_block_hash, parent's block_hash) for
    every buildable combination: both fields start from one random 256-byte
    text without a NUL, get their NULs at pc and pp, then the child's field one
    differing byte."""
    rng = random.Random(seed)
    out = []
    for pc in NUL_AT:
        for pp in NUL_AT:
            for kind in DIFF_AT:
                pos = None
                if kind != "none":
                    pos = _diff_position(kind, pc, pp)
                    if pos is None:
                        continue
                text = bytearray(rng.randrange(1, 256) for _ in range(256))
                a, b = bytearray(text), bytearray(text)
                if pc is not None:
                    a[pc] = 0
                if pp is not None:
                    b[pp] = 0
                if pos is not None:
                    a[pos] = a[pos] % 255 + 1  # another byte, never NUL
                out.append((pc, pp, kind, bytes(a), bytes(b)))
    return out


def link_differs(a: bytes, b: bytes) -> bool:
    """check_chain's compare of the two fields as C strings (node.cpp:117-125)."""
    return a.split(b"\0")[0] != b.split(b"\0")[0]


def link_chain(cases, seed: int = 8):
    """One flat chain, tip first: blocks 2k and 2k + 1 are case k's child and
    parent.  Random nonces, nothing mined, stored hashes as the case wants them."""
    rng = random.Random(seed)
    arr = (Block * (2 * len(cases)))()
    for k, (_, _, _, a, b) in enumerate(cases):
        nonce = bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789") for _ in range(9))
        arr[2 * k] = make_block(1000 + k, rng.randrange(8), 0, 1_700_000_000 + k, prev=a, nonce=nonce,
                                block_hash=bytes(rng.randrange(256) for _ in range(256)))
        arr[2 * k + 1] = make_block(999 + k, rng.randrange(8), 0, 1_700_000_000 + k,
                                    prev=bytes(rng.randrange(256) for _ in range(256)), nonce=nonce[::-1], block_hash=b)
    return arr


# ---- the hex matrix ----
HEX_SEED, HEX_BLOCKS = 40, 400  # with this seed every hex value occurs at every text position
HEX_KINDS = ("next_digit", "uppercase", "nul", "bit7", "slash", "colon", "backtick", "g")
# blocks to corrupt first: lanes 0, 31 and 63 of workgroup 0, lane 32 of workgroup 1; then every
# second block, so that no corrupted block is another one's parent
SLOTS = (0, 31, 63, 96) + tuple(range(130, HEX_BLOCKS - 1, 2))


def hex_chain():
    return vu.build_chain(HEX_BLOCKS, 0, seed=HEX_SEED)


def replacement(kind: str, c: int):
    """The byte that replaces the hex character c, or None if `kind` has none for it."""
    if kind == "next_digit":
        return b"0123456789abcdef"[(int(chr(c), 16) + 1) % 16]
    if kind == "uppercase":
        return c - 32 if c >= ord("a") else None
    return {"nul": 0, "bit7": c | 0x80, "slash": ord("/"), "colon": ord(":"), "backtick": ord("`"), "g": ord("g")}[kind]


def corrupt_hex(chain, kind: str):
    """A copy of `chain` in which, for each of the 64 text positions, another
    block has that character of its block_hash replaced; and {block: position}."""
    out = vu.copy_chain(chain)
    used = {}
    for p in range(64):
        for i in SLOTS:
            if i in used:
                continue
            raw = bytearray(field(out[i], "block_hash"))
            r = replacement(kind, raw[p])
            if r is None:
                continue
            assert r != raw[p]
            raw[p] = r
            set_field(out[i], "block_hash", bytes(raw))
            used[i] = p
            break
        else:
            raise AssertionError(f"no block left for position {p} of {kind}")
    return out, used


def set_hash_byte(chain, i: int, pos: int, value: int) -> None:
    ctypes.memset(ctypes.addressof(chain[i]) + Block.block_hash.offset + pos, value, 1)

