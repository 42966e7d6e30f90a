#!/usr/bin/env python3
"""Records six independent templates MINED through the REFERENCE's own
block_to_hash and solves_problem (oracle/_ref/libref_O2.so, made by
`make -C oracle ref` where the reference's sources are present), so that the
host statement of pow_mine_batch (mpi_blockchain_amd.block.mine_batch) is
pinned to the reference where its build is absent:

  mined_batch.json
    parent      the block every template was refreshed from (node.cpp:292-299):
                index 0, a 64-character block_hash
    difficulty  8, ctr_start 0
    templates   6 templates on that parent, as N ranks build them
                (node.cpp:292-302): they differ in node_owner_number and
                created_at.  One has created_at above 2^32 (hashed as one
                byte, trap T2); one has its index moved to 300 (hashed as one
                byte, trap T1); one has a 256-byte previous_block_hash with a
                non-zero tail behind the text's NUL (all 256 bytes are
                hashed, trap T5).
    counters    per template, the LOWEST counter from 0 whose nonce solves it
    mined       per template, the nonce and the 64 hex characters of its digest

Only field values and counters are recorded.

The reference's solves_problem has its difficulty compiled in
(DEFAULT_DIFFICULTY = 9 bits, block.h:6).  Eight bits are asked of it as the
first two hex characters of the digest followed by '0': its ninth binary digit
is then the '0''s first, so it answers for the first eight alone.

    python tests/golden/gen_mined_batch.py      # needs oracle/_ref
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from oracle.oracle import OBlock, RefLib, make_oblock, py_nonce_from_counter, raw_field  # noqa: E402

DIFFICULTY = 8
PARENT_HASH = b"00c3a1f0e2d4b5968778695a4b3c2d1e0ff1e2d3c4b5a69788796a5b4c3d2e1f"
TAIL = bytes(1 + (7 * i) % 255 for i in range(256 - 65))  # behind the text's NUL: no zero byte
# (index, node_owner_number, created_at, previous_block_hash)
TEMPLATES = [
    (1, 0, 1_700_000_000, PARENT_HASH),
    (1, 1, 1_700_000_000, PARENT_HASH),
    (1, 2, 1_700_000_003, PARENT_HASH),
    (1, 3, (1 << 32) + 55, PARENT_HASH),
    (300, 4, 1_700_000_009, PARENT_HASH),
    (1, 19, 1_700_000_011, PARENT_HASH + b"\0" + TAIL),
]


def main():
    R = RefLib("O2")
    assert R.default_difficulty == 9 and DIFFICULTY == 8
    assert len(PARENT_HASH) == 64 and len(PARENT_HASH + b"\0" + TAIL) == 256
    templates, counters, mined = [], [], []
    for index, owner, created_at, prev in TEMPLATES:
        b = make_oblock(index, owner, DIFFICULTY, created_at, prev)
        ctr = 0
        while True:
            ctypes.memmove(ctypes.addressof(b) + OBlock.nonce.offset, py_nonce_from_counter(ctr), 10)
            hx = R.block_to_hash(b)
            if R.solves_problem(hx[:2] + "0"):
                break
            ctr += 1
        templates.append({"index": index, "node_owner_number": owner, "difficulty": DIFFICULTY,
                          "created_at": created_at, "previous_block_hash_hex": prev.hex()})
        counters.append(ctr)
        mined.append({"nonce_hex": raw_field(b, "nonce").hex(), "block_hash": hx})
    out = {"generator": "tests/golden/gen_mined_batch.py",
           "reference": "oracle/_ref/libref_O2.so (the reference's own block_to_hash and solves_problem)",
           "difficulty": DIFFICULTY, "ctr_start": 0,
           "parent": {"index": 0, "block_hash_hex": PARENT_HASH.hex()},
           "templates": templates, "counters": counters, "mined": mined}
    with open(os.path.join(HERE, "mined_batch.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
    print("wrote mined_batch.json:", len(templates), "templates, counters", counters)


if __name__ == "__main__":
    main()
