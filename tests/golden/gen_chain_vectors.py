#!/usr/bin/env python3
"""Records a 70-block chain whose block_hash strings come from the REFERENCE's
own block_to_hash (oracle/_ref/libref_O2.so, made by `make -C oracle ref`
where the reference's sources are present), so that the chain-verification
tests check against the reference's hashing where its build is absent:

  chain_vectors.json
    difficulty  the leading zero bits every block of the chain has (4)
    chain       70 blocks, tip first: the integer fields, nonce and
                previous_block_hash as hex (trailing NULs trimmed) and the
                reference's block_hash text.  It holds indices above 255 and
                one created_at above 2^32 (both are hashed as one byte, traps
                T1/T2), and one block whose previous_block_hash has non-zero
                bytes after its NUL: they are hashed (block_to_str takes all
                256 bytes) and ignored by the link (a C-string compare).

    python tests/golden/gen_chain_vectors.py      # needs oracle/_ref

mpi_blockchain_amd.block.verify_chain gives status 0 for every block of it
(tests/test_verify_host.py).
"""
import ctypes
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from oracle.oracle import OBlock, RefLib, make_oblock, py_nonce_from_counter, raw_field  # noqa: E402

N = 70
DIFFICULTY = 4
FIRST_INDEX = 201          # 201..270: crosses 255
BIG_TIME_AT = 40           # this block's created_at is above 2^32
TAIL_AT = 23               # this block's previous_block_hash has bytes after its NUL


def main():
    R = RefLib("O2")
    rng = random.Random(70)
    chain = []
    prev = b""
    for j in range(N):
        created = (1 << 32) + 123_456_789 if j == BIG_TIME_AT else 1_700_000_000 + 11 * j
        if j == TAIL_AT:
            prev = prev[:65] + b"left over after the NUL" + prev[88:]
        ctr = rng.randrange(62 ** 9 - (1 << 32))
        while True:
            b = make_oblock(FIRST_INDEX + j, rng.randrange(8), DIFFICULTY, created, prev, py_nonce_from_counter(ctr))
            hx = R.block_to_hash(b)
            if hx[0] == "0":  # DIFFICULTY = 4 bits = one hex digit
                break
            ctr += 1
        ctypes.memmove(ctypes.addressof(b) + OBlock.block_hash.offset, hx.encode() + b"\0", 65)
        chain.append(b)
        prev = raw_field(b, "block_hash")
    out = {"generator": "tests/golden/gen_chain_vectors.py",
           "reference": "oracle/_ref/libref_O2.so (the reference's own block_to_hash)",
           "difficulty": DIFFICULTY,
           "chain": [{"index": b.index, "node_owner_number": b.node_owner_number, "difficulty": b.difficulty,
                      "created_at": b.created_at, "nonce_hex": raw_field(b, "nonce").hex(),
                      "previous_block_hash_hex": raw_field(b, "previous_block_hash").rstrip(b"\0").hex(),
                      "block_hash": raw_field(b, "block_hash").split(b"\0", 1)[0].decode()}
                     for b in reversed(chain)]}
    with open(os.path.join(HERE, "chain_vectors.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
    print("wrote chain_vectors.json:", len(chain), "blocks, indices", chain[0].index, "..", chain[-1].index)


if __name__ == "__main__":
    main()
