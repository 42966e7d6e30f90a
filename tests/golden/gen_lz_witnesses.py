"""Generate tests/golden/lz_witnesses.json: counters whose digests sit on the
two sides of the 32-bit difficulty seam, where every kernel changes its
proof-of-work test (K1/K1': H0 <= thr up to d = 32, the full-width count above;
K4: H0 <= thr, and the host loop above 32; K3: the count over eight words).

    python tests/golden/gen_lz_witnesses.py          # the "seam" rows (CPU, hashlib)
    python tests/golden/gen_lz_witnesses.py --chain  # + the "chain" rows (needs the GPU)

"seam": three of the d = 25 solutions that the committed 2^32 fingerprints
(fingerprints_2p32*.json, "first") list for the templates S0, S1 and S2 of
golden.json happen to have 31, 32 and 33 leading zero bits.  This script only
re-derives their digests with hashlib and refuses to write anything else.

"chain": pow_mine_chain's template carries difficulty = diff_bits in the
hashed header, so the rows above do not apply to it.  For a fixed parent, owner
and created_at and each d in 31, 32, 33 the GPU sweeps whole 2^32 windows of
the template (difficulty field = d) at d - 1 bits until it has one counter with
at least d leading zero bits ("solves") and one with exactly d - 1 ("misses")
whose 2,048-counter window holds no solution at d.  The search is only a
search: every digest written is hashlib's, and the tests check every row with
hashlib again before they use it.
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.oracle import py_block_to_str, py_nonce_from_counter  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "lz_witnesses.json")
SEAM = [("S2", 215925281, 33), ("S1", 142414799, 32), ("S0", 25949249075, 31)]
# pow_mine_chain's inputs for the "chain" rows: initialize_first_block's genesis as the parent
PARENT = {"index": 0, "node_owner_number": 0, "difficulty": 9, "created_at": 1_699_999_990}
OWNER, CREATED_AT = 5, 1_700_000_123
BEFORE, WINDOW = 1000, 2048  # a witness's window is [counter - BEFORE, counter - BEFORE + WINDOW)


def digest_of(index, owner, difficulty, created_at, prev, ctr):
    return hashlib.sha256(py_block_to_str(index, owner, difficulty, created_at, py_nonce_from_counter(ctr),
                                          prev)).digest()


def lz_of(digest):
    return 256 - int.from_bytes(digest, "big").bit_length()


def seam_rows():
    with open(os.path.join(HERE, "golden.json")) as f:
        templates = {t["name"]: t for t in json.load(f)["templates"]}
    rows = []
    for name, ctr, lz in SEAM:
        t = templates[name]
        dg = digest_of(t["index"], t["node_owner_number"], t["difficulty"], t["created_at"],
                       bytes.fromhex(t["previous_block_hash_hex"]), ctr)
        assert lz_of(dg) == lz, (name, ctr, lz_of(dg))
        rows.append({"template": name, "counter": ctr, "leading_zeros": lz, "digest": dg.hex()})
    return rows


def chain_rows(max_windows=64):
    from mpi_blockchain_amd.block import field, make_block
    from mpi_blockchain_amd.miner import GpuMiner, refresh_template

    parent = make_block(PARENT["index"], PARENT["node_owner_number"], PARENT["difficulty"], PARENT["created_at"])
    rows, searched = [], {}
    with GpuMiner(0) as m:
        for d in (31, 32, 33):
            tmpl = refresh_template(parent, OWNER, d, CREATED_AT)
            prev = field(tmpl, "previous_block_hash")

            def lz(ctr):
                return lz_of(digest_of(tmpl.index, OWNER, d, CREATED_AT, prev, ctr))

            solves = misses = None
            for w in range(max_windows):
                start = w << 32
                found = [start + int(r) for r in m.sweep(tmpl, start, 1 << 32, d - 1)]
                zs = {c: lz(c) for c in found}
                assert all(z >= d - 1 for z in zs.values()), (d, zs)
                for c in found:
                    if zs[c] >= d and solves is None and c >= BEFORE:
                        solves = c
                    lonely = not any(zs[o] >= d and c - BEFORE <= o < c - BEFORE + WINDOW for o in found)
                    if zs[c] == d - 1 and misses is None and c >= BEFORE and lonely:
                        misses = c
                searched[str(d)] = w + 1
                if solves is not None and misses is not None:
                    break
            assert solves is not None and misses is not None, (d, solves, misses)
            for kind, c in (("solves", solves), ("misses", misses)):
                dg = digest_of(tmpl.index, OWNER, d, CREATED_AT, prev, c)
                rows.append({"difficulty": d, "kind": kind, "counter": c, "leading_zeros": lz_of(dg),
                             "digest": dg.hex()})
    return {"parent": PARENT, "owner": OWNER, "created_at": CREATED_AT, "before": BEFORE, "window": WINDOW,
            "windows_searched": searched, "witnesses": rows}


if __name__ == "__main__":
    out = {"seam": seam_rows()}
    if "--chain" in sys.argv[1:]:
        out["chain"] = chain_rows()
    elif os.path.exists(OUT):
        with open(OUT) as f:
            out["chain"] = json.load(f).get("chain")
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
