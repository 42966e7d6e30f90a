#!/usr/bin/env python3
"""Records what a solo rank of the REFERENCE mines from a given seed, made by
the reference's own code (oracle/_ref through RefLib): ref_srand(seed), then per
block the loop of node.cpp:292-318 with created_at pinned: refresh the template
on the tip, gen_random_nonce, block_to_hash, solves_problem (the reference's
compile-time difficulty, 9), and on success strcpy of the hash and on to the
next block; the stream of rand() runs on across the blocks.

  rand_replay.json
    replays  per (seed, template): the parent (552 bytes, hex), the rank, the
             created_at of each block, and for each of the 3 linked blocks the
             trial at which it solved (the count of gen_random_nonce calls
             before it, from the srand) and its 552 bytes (hex);
    nonces   per seed: the first 64 gen_random_nonce results after srand(seed).

The parent of a replay is made from a golden template S: the template's own
fields, index - 1, and S's previous_block_hash as its block_hash, so that the
first refreshed template hashes what S hashes (S2: the non-zero tail of
previous_block_hash, trap T5, which every later block inherits).

    python tests/golden/gen_rand_replay.py      # needs oracle/_ref
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from oracle.oracle import OBlock, RefLib, make_oblock  # noqa: E402

N_BLOCKS = 3
# 0 counts as 1; the sign bit; all ones; time(NULL) + mpi_rank (node.cpp:386); and
# the sign bit's two neighbours, whose first Lehmer step gives 0: r[1..30] are all zero
SEEDS = (0, 1, 0x80000000, 0xFFFFFFFF, 1700000000 + 3, 0x7FFFFFFF, 0x80000001)
PAIRS = ((0, "S0"), (1, "S1"), (0x80000000, "S2"), (0xFFFFFFFF, "S0"), (1700000000 + 3, "S2"))


def raw(b: OBlock) -> bytes:
    return ctypes.string_at(ctypes.addressof(b), ctypes.sizeof(b))


def parent_of(t: dict) -> OBlock:
    p = make_oblock(t["index"] - 1, t["node_owner_number"], t["difficulty"], t["created_at"], b"")
    ctypes.memmove(ctypes.addressof(p) + OBlock.block_hash.offset, bytes.fromhex(t["previous_block_hash_hex"]), 256)
    return p


def replay(R: RefLib, seed: int, t: dict) -> dict:
    last = parent_of(t)
    rank = t["node_owner_number"]
    times = [(t["created_at"] + 17 * k) & 0xFFFFFFFFFFFFFFFF for k in range(N_BLOCKS)]
    out = {"seed": seed, "template": t["name"], "rank": rank, "difficulty": R.default_difficulty,
           "created_at": times, "parent_hex": raw(last).hex(), "blocks": []}
    R.L.ref_srand(seed)
    trial = 0
    for k in range(N_BLOCKS):
        while True:
            b = OBlock()  # node.cpp:292-299
            ctypes.pointer(b)[0] = last
            b.index = (last.index + 1) & 0xFFFFFFFF
            b.node_owner_number = rank
            b.difficulty = R.default_difficulty
            b.created_at = times[k]
            ctypes.memmove(ctypes.addressof(b) + OBlock.previous_block_hash.offset,
                           ctypes.addressof(b) + OBlock.block_hash.offset, 256)
            ctypes.memmove(ctypes.addressof(b) + OBlock.nonce.offset, R.gen_random_nonce(), 10)  # node.cpp:302
            hx = R.block_to_hash(b)
            trial += 1
            if R.solves_problem(hx):
                ctypes.memmove(ctypes.addressof(b) + OBlock.block_hash.offset, hx.encode() + b"\0", 65)  # node.cpp:318
                out["blocks"].append({"trial": trial - 1, "block_hex": raw(b).hex()})
                last = b
                break
    out["total_trials"] = trial
    return out


def main():
    with open(os.path.join(HERE, "golden.json")) as f:
        templates = {t["name"]: t for t in json.load(f)["templates"]}
    R = RefLib("O2")
    assert R.default_difficulty == 9
    replays = [replay(R, seed, templates[name]) for seed, name in PAIRS]
    nonces = {}
    for seed in SEEDS:
        R.L.ref_srand(seed)
        nonces[str(seed)] = [bytes(R.gen_random_nonce()).hex() for _ in range(64)]
    out = {"generator": "tests/golden/gen_rand_replay.py",
           "reference": "oracle/_ref/libref_O2.so (the reference's own gen_random_nonce, block_to_hash and solves_problem)",
           "replays": replays, "nonces": nonces}
    with open(os.path.join(HERE, "rand_replay.json"), "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
    print("wrote rand_replay.json:", [(r["seed"], r["template"], [b["trial"] for b in r["blocks"]]) for r in replays])


if __name__ == "__main__":
    main()
