"""Generate tests/golden/deep_stretch.json: a long stretch of counters that the
CPU oracle certifies empty at d = 30, ending in a solution.

The hashlib statements of pow_mine_chain, pow_mine_batch and pow_mine_race hash
every counter below the answer in Python, so their tests keep the winning
relative counter small.  This fixture supplies what they cannot: a window
[empty_from, counter) of at least 62^5 + 2^20 counters without a solution at 30
bits, so that a fused kernel started anywhere in it must walk to `counter` and
every base-62 digit of its relative counter is reached.

Template: pow_mine_chain's refresh of the chain inputs of lz_witnesses.json at
difficulty 30 (parent index 0, owner 0, difficulty 9, created_at 1,699,999,990
with an all-zero block_hash; child index 1, owner 5, created_at 1,700,000,123,
previous hash = all 256 bytes of the parent's block_hash).  The difficulty is
part of the hashed header, so it is fixed before the sweep.

The sweep (oracle/pow_oracle.c, oracle_sweep_lz) goes forward from counter 0 in
chunks at 24 bits and records (counter, leading zero bits) of every hit.  It
stops at the first solution b with >= 30 bits that has no other such solution
in the 62^5 + 2^20 counters before it; a is the solution before b, or -1.  Past
2^34 counters it adds 1 to created_at and starts again.  The stretch is capped
at 2^32 - 1 counters.  Every digest written is hashlib's.  CPU only; 5 to 15
minutes on 8 threads.

    python tests/golden/gen_deep_stretch.py [threads]
"""
import ctypes, hashlib, json, os, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.oracle import OBlock, Oracle, make_oblock, py_block_to_str, py_nonce_from_counter  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
PARENT = {"index": 0, "node_owner_number": 0, "difficulty": 9, "created_at": 1_699_999_990}
OWNER, CREATED_AT, D, THRESHOLD = 5, 1_700_000_123, 30, 24
PREV = bytes(256)  # the parent's block_hash: make_block leaves it zero
NEED = 62 ** 5 + 2 ** 20
CHUNK, GIVE_UP, CAP = 1 << 28, 1 << 34, (1 << 32) - 1

threads = int(sys.argv[1]) if len(sys.argv) > 1 else 8
L = Oracle().L
L.oracle_sweep_lz.argtypes = [ctypes.POINTER(OBlock), ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint,
                              ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint8),
                              ctypes.c_size_t, ctypes.c_int]
L.oracle_sweep_lz.restype = ctypes.c_size_t


def sweep(tmpl, start, count):
    """[(counter, lz)] of the hits at THRESHOLD bits in [start, start + count), ascending."""
    cap = (count >> THRESHOLD) * 8 + 4096
    ctr, lz = np.zeros(cap, np.uint32), np.zeros(cap, np.uint8)
    n = L.oracle_sweep_lz(ctypes.byref(tmpl), start, count, THRESHOLD,
                          ctr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                          lz.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), cap, threads)
    assert n <= cap
    return [(start + int(c), int(z)) for c, z in zip(ctr[:n], lz[:n])]


def search(created_at):
    """(a, b, rows, swept) of the first qualifying stretch, or None past GIVE_UP."""
    tmpl = make_oblock(PARENT["index"] + 1, OWNER, D, created_at, PREV)
    rows, a, at = [], -1, 0
    while at < GIVE_UP:
        for c, z in sweep(tmpl, at, CHUNK):
            rows.append((c, z))
            if z >= D:
                if c - a - 1 >= NEED:
                    return a, c, rows, at + CHUNK
                a = c
        at += CHUNK
        print(f"created_at {created_at}: swept {at:,}, last solution {a:,}, {time.time() - t0:.0f} s", flush=True)
    return None


t0 = time.time()
tries, created_at = 0, CREATED_AT
while True:
    tries += 1
    got = search(created_at)
    if got:
        break
    created_at += 1
a, b, rows, swept = got
empty_from = max(a + 1, b - CAP)


def digest_of(ctr):
    return hashlib.sha256(py_block_to_str(PARENT["index"] + 1, OWNER, D, created_at, py_nonce_from_counter(ctr),
                                          PREV)).digest()


def lz_of(digest):
    return 256 - int.from_bytes(digest, "big").bit_length()


rows = [(c, z) for c, z in rows if empty_from <= c <= b]
for c, z in rows:
    assert lz_of(digest_of(c)) == z, (c, z)
assert [c for c, z in rows if z >= D] == [b] and b - empty_from >= NEED
out = {"parent": PARENT, "owner": OWNER, "created_at": created_at, "difficulty": D, "threshold": THRESHOLD,
       "tries": tries, "swept": swept, "seconds": round(time.time() - t0, 1), "previous_solution": a,
       "empty_from": empty_from, "counter": b, "digest": digest_of(b).hex(),
       "leading_zeros": lz_of(digest_of(b)), "rows": [[c, z] for c, z in rows]}
with open(os.path.join(HERE, "deep_stretch.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps({k: v for k, v in out.items() if k != "rows"}), len(rows), "rows")
