#!/usr/bin/env python3
"""Cost of "is this chain valid?" on one MI355X and on the same box's CPU.

For chains of n = 5 ... 200, 4,096, 2^16 and 2^20 blocks (valid, difficulty 0, so
no mining is needed to build them; the work test runs at every difficulty):

  gpu call     pow_verify_chain, host clock around the call (it returns after
               its bounded wait on the stream: copy in, kernel, verdict out)
  gpu kernel   kernel_ms of pow_get_stats (HIP events around the launches)
  ref -O2      the reference's own block_to_hash in a C loop over n blocks
               (oracle/_ref/libref_O2.so: ref_sweep, i.e. block_to_hash plus
               the nonce write and solves_problem per block), one CPU thread
  hash_blocks  the route without pow_verify_chain: pow_hash_blocks (hex out)
               plus the comparisons of hex, link, index and work in Python

Median of 21 calls after 3 warm-up calls (5 after 1 where one call takes more
than a second: the CPU routes at 2^20).  Writes the table to
profiles/verify_chain/README.md (or --out) and prints it.

    python tools/verify_chain_bench.py [--out FILE] [--sizes 5,200,...]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from mpi_blockchain_amd._lib import check  # noqa: E402
from mpi_blockchain_amd.block import field  # noqa: E402
from mpi_blockchain_amd.miner import GpuMiner  # noqa: E402
from oracle.oracle import OBlock, RefLib  # noqa: E402
from verify_util import build_chain, copy_chain  # noqa: E402

SIZES = (5, 16, 32, 64, 128, 200, 1024, 4096, 1 << 16, 1 << 20)  # the five of the issue, and more below 200


def median_ms(fn, slow: bool):
    reps, warm = (5, 1) if slow else (21, 3)
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts), reps


def python_checks(chain, hexes: bytes, difficulty: int) -> int:
    """What a caller of pow_hash_blocks has to do by hand; returns flagged blocks."""
    n = len(chain)
    bad = 0
    stored = [field(b, "block_hash") for b in chain]
    for i, b in enumerate(chain):
        hx = hexes[65 * i: 65 * i + 64]
        ok = stored[i][:64] == hx and stored[i][64] == 0 and 256 - int(hx, 16).bit_length() >= difficulty
        if ok and i < n - 1:
            ok = (field(b, "previous_block_hash").split(b"\0", 1)[0] == stored[i + 1].split(b"\0", 1)[0]
                  and (b.index - 1) & 0xFFFFFFFF == chain[i + 1].index)
        bad += not ok
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_chain", "README.md"))
    ap.add_argument("--sizes", default=",".join(map(str, SIZES)))
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]
    R = RefLib("O2")
    t0 = time.perf_counter()
    full = build_chain(max(sizes), 0, seed=9)
    print(f"built {max(sizes)} blocks in {time.perf_counter() - t0:.1f} s", flush=True)
    rows = []
    with GpuMiner(0) as m:
        m.warmup()
        info = m.device_info()
        for n in sizes:
            chain = copy_chain(full, 0, n)  # any slice of a valid chain is a valid chain
            first, bad = ctypes.c_size_t(), ctypes.c_size_t()
            kernel = []

            def gpu():
                rc = check(m.L.pow_verify_chain(m.ctx, chain, n, 0, None, ctypes.byref(first), ctypes.byref(bad)), m.L)
                assert rc == 1 and first.value == n and bad.value == 0
                kernel.append(m.stats()["kernel_ms"])

            g = median_ms(gpu, False)
            k = statistics.median(kernel[-g[3]:])
            tmpl = OBlock()
            ctypes.memmove(ctypes.addressof(tmpl), ctypes.addressof(chain[0]), ctypes.sizeof(OBlock))
            c = median_ms(lambda: R.sweep(tmpl, 0, n, cap=1), n >= 1 << 19)
            hexes = ctypes.create_string_buffer(65 * n)

            def route():
                check(m.L.pow_hash_blocks(m.ctx, chain, n, None, hexes), m.L)
                assert python_checks(chain, hexes.raw, 0) == 0

            h = median_ms(route, n >= 1 << 19)
            rows.append((n, g, k, c, h))
            print(f"n={n}: gpu call {g[0]:.3f} ms (kernel {k:.3f}), ref -O2 {c[0]:.3f} ms, hash_blocks route {h[0]:.3f} ms",
                  flush=True)
    cross = next((n for n, g, _, c, _ in rows if g[0] < c[0]), None)
    lines = ["# pow_verify_chain: cost per call", "",
             f"Measured by `tools/verify_chain_bench.py` on {info['name']} ({info['cu_count']} CUs) and one CPU thread "
             "of the same box.  Valid chains, difficulty 0.  Median [min, max] in ms over the calls given; "
             "see the tool's docstring for what each column times.", "",
             "| n | gpu call ms | gpu kernel ms | us per block (gpu call) | ref -O2 loop ms | us per block (ref) | "
             "pow_hash_blocks + Python ms | gpu call vs ref |",
             "|---|---|---|---|---|---|---|---|"]
    for n, g, k, c, h in rows:
        lines.append(f"| {n:,} | {g[0]:.3f} [{g[1]:.3f}, {g[2]:.3f}] x{g[3]} | {k:.3f} | {g[0] * 1e3 / n:.3f} | "
                     f"{c[0]:.3f} [{c[1]:.3f}, {c[2]:.3f}] x{c[3]} | {c[0] * 1e3 / n:.3f} | "
                     f"{h[0]:.3f} [{h[1]:.3f}, {h[2]:.3f}] x{h[3]} | {c[0] / g[0]:.2f}x |")
    lines += ["", ("Crossover: the GPU call is faster than the reference's -O2 loop from n = "
                   f"{cross:,} of the sizes measured (and slower below)." if cross is not None else
                   "The GPU call is slower than the reference's -O2 loop at every size measured."), ""]
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
