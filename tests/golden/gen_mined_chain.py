#!/usr/bin/env python3
"""Records a chain MINED through the REFERENCE's own block_to_hash and
solves_problem (oracle/_ref/libref_O2.so, made by `make -C oracle ref` where
the reference's sources are present), so that the host statement of
pow_mine_chain (mpi_blockchain_amd.block.mine_chain) is pinned to the
reference where its build is absent:

  mined_chain.json
    parent      the genesis block of initialize_first_block (node.cpp:361-372):
                index 0, owner 0, difficulty 9, block_hash zeroed
    difficulty  8, owner 3, created_at one fixed value per block (one of them
                above 2^32: hashed as one byte, trap T2), ctr_start 0
    chain       6 blocks, tip first: the integer fields, the nonce, and
                previous_block_hash / block_hash as hex of all 256 bytes with
                the trailing NULs trimmed

Each block is the reference's template refresh (node.cpp:292-299: the last
block copied, index + 1, owner, difficulty, created_at, memcpy of all 256
bytes of its block_hash into previous_block_hash), sealed by the LOWEST
counter from 0 whose nonce solves it, with strcpy of the hash (node.cpp:318).

The reference's solves_problem has its difficulty compiled in
(DEFAULT_DIFFICULTY = 9 bits, block.h:6).  Eight bits are asked of it as the
first two hex characters of the digest followed by '0': its ninth binary digit
is then the '0''s first, so it answers for the first eight alone.

    python tests/golden/gen_mined_chain.py      # needs oracle/_ref
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from oracle.oracle import HASH_SIZE, OBlock, RefLib, make_oblock, py_nonce_from_counter, raw_field  # noqa: E402

N = 6
DIFFICULTY = 8
OWNER = 3
CREATED_AT = [1_700_000_000, 1_700_000_007, (1 << 32) + 55, 1_700_000_021, 1_700_000_300, 1_700_000_301]
PARENT = dict(index=0, node_owner_number=0, difficulty=9, created_at=1_699_999_990)


def refresh(last: OBlock, owner: int, difficulty: int, created_at: int) -> OBlock:
    """node.cpp:292-299."""
    b = OBlock()
    ctypes.memmove(ctypes.addressof(b), ctypes.addressof(last), ctypes.sizeof(OBlock))
    b.index = (last.index + 1) & 0xFFFFFFFF
    b.node_owner_number = owner
    b.difficulty = difficulty
    b.created_at = created_at
    ctypes.memmove(ctypes.addressof(b) + OBlock.previous_block_hash.offset,
                   ctypes.addressof(last) + OBlock.block_hash.offset, HASH_SIZE)
    return b


def entry(b: OBlock) -> dict:
    return {"index": b.index, "node_owner_number": b.node_owner_number, "difficulty": b.difficulty,
            "created_at": b.created_at, "nonce_hex": raw_field(b, "nonce").hex(),
            "previous_block_hash_hex": raw_field(b, "previous_block_hash").rstrip(b"\0").hex(),
            "block_hash_hex": raw_field(b, "block_hash").rstrip(b"\0").hex()}


def main():
    R = RefLib("O2")
    assert R.default_difficulty == 9 and DIFFICULTY == 8
    last = make_oblock(PARENT["index"], PARENT["node_owner_number"], PARENT["difficulty"], PARENT["created_at"], b"")
    parent = last
    chain, counters = [], []
    for k in range(N):
        b = refresh(last, OWNER, DIFFICULTY, CREATED_AT[k])
        ctr = 0
        while True:
            ctypes.memmove(ctypes.addressof(b) + OBlock.nonce.offset, py_nonce_from_counter(ctr), 10)
            hx = R.block_to_hash(b)
            if R.solves_problem(hx[:2] + "0"):
                break
            ctr += 1
        ctypes.memmove(ctypes.addressof(b) + OBlock.block_hash.offset, hx.encode() + b"\0", 65)  # strcpy
        chain.append(b)
        counters.append(ctr)
        last = b
    out = {"generator": "tests/golden/gen_mined_chain.py",
           "reference": "oracle/_ref/libref_O2.so (the reference's own block_to_hash and solves_problem)",
           "difficulty": DIFFICULTY, "owner": OWNER, "created_at": CREATED_AT, "ctr_start": 0,
           "parent": entry(parent), "counters": list(reversed(counters)),
           "chain": [entry(b) for b in reversed(chain)]}
    with open(os.path.join(HERE, "mined_chain.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
    print("wrote mined_chain.json:", len(chain), "blocks, counters", counters)


if __name__ == "__main__":
    main()
