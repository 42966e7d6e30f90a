#!/usr/bin/env python3
"""Cost of "which of these chains are valid?" on one MI355X and on the same
box's CPU, for batches of n_chains x length blocks (valid chains, difficulty
0, so no mining is needed to build them; the work test runs at every
difficulty):

  chains call  pow_verify_chains over the whole batch, host clock around the
               call (offsets and structs in, one launch per 2^16 blocks,
               verdicts out, the fork choice)
  kernel       kernel_ms of pow_get_stats for that call (HIP events)
  chain loop   pow_verify_chain called chain by chain over the same buffer, in
               the same process: one launch boundary per chain
  ref -O2      the reference's own block_to_hash in a C loop over as many
               blocks (oracle/_ref/libref_O2.so: ref_sweep, i.e. block_to_hash
               plus the nonce write and solves_problem per block), one CPU thread

Median of 21 calls (or --calls) after 3 warm-up calls.  Writes the table to
profiles/verify_chains/README.md (or --out) and prints it; --json FILE keeps
every call's time of the two GPU columns, for comparing two builds.

    python tools/verify_chains_bench.py [--calls 21] [--out FILE] [--json FILE] [--shapes 2x5,64x200,...]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from mpi_blockchain_amd._lib import Block, check  # noqa: E402
from mpi_blockchain_amd.miner import GpuMiner  # noqa: E402
from oracle.oracle import OBlock, RefLib  # noqa: E402
from verify_util import build_chain  # noqa: E402

SHAPES = ((2, 5), (16, 5), (64, 5), (1024, 5), (64, 200), (1 << 14, 5))
REPS, WARM = 21, 3


def median_ms(fn, samples=None):
    for _ in range(WARM):
        fn()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    if samples is not None:
        samples.extend(ts)
    return statistics.median(ts), min(ts), max(ts)


def main():
    global REPS
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_chains", "README.md"))
    ap.add_argument("--shapes", default=",".join(f"{n}x{k}" for n, k in SHAPES))
    ap.add_argument("--calls", type=int, default=REPS)
    ap.add_argument("--json")
    args = ap.parse_args()
    REPS = args.calls
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    R = RefLib("O2")
    most = max(n * k for n, k in shapes)
    t0 = time.perf_counter()
    full = build_chain(most, 0, seed=9)  # every slice of a valid chain is a valid chain: the batches are slices
    print(f"built {most} blocks in {time.perf_counter() - t0:.1f} s", flush=True)
    size = ctypes.sizeof(Block)
    rows, samples = [], []
    with GpuMiner(0) as m:
        m.warmup()
        info = m.device_info()
        L, ctx = m.L, m.ctx
        for n, k in shapes:
            total = n * k
            lengths = (ctypes.c_uint32 * n)(*[k] * n)
            first, bad = (ctypes.c_uint32 * n)(), (ctypes.c_uint32 * n)()
            best = ctypes.c_size_t()
            kernel = []

            def chains_call():
                rc = check(L.pow_verify_chains(ctx, full, lengths, n, 0, None, first, bad, ctypes.byref(best)), L)
                assert rc == 1 and best.value == 0
                kernel.append(m.stats()["kernel_ms"])

            tips = [ctypes.cast(ctypes.byref(full, c * k * size), ctypes.POINTER(Block)) for c in range(n)]
            f1, b1 = ctypes.c_size_t(), ctypes.c_size_t()
            pf, pb = ctypes.byref(f1), ctypes.byref(b1)
            verify_chain = L.pow_verify_chain

            def chain_loop():
                ok = 0
                for tip in tips:
                    ok += verify_chain(ctx, tip, k, 0, None, pf, pb)
                assert ok == n

            sample = {"chains": n, "length": k, "chains_call_ms": [], "chain_loop_ms": []}
            samples.append(sample)
            g = median_ms(chains_call, sample["chains_call_ms"])
            kern = statistics.median(kernel[-REPS:])
            assert list(first) == [k] * n and not any(bad)
            lp = median_ms(chain_loop, sample["chain_loop_ms"])
            tmpl = OBlock()
            ctypes.memmove(ctypes.addressof(tmpl), ctypes.addressof(full[0]), ctypes.sizeof(OBlock))
            c = median_ms(lambda: R.sweep(tmpl, 0, total, cap=1))
            rows.append((n, k, g, kern, lp, c))
            print(f"{n} x {k}: chains call {g[0]:.3f} ms (kernel {kern:.3f}), chain loop {lp[0]:.3f} ms, "
                  f"ref -O2 {c[0]:.3f} ms", flush=True)
    lines = ["# pow_verify_chains: cost per call", "",
             f"Measured by `tools/verify_chains_bench.py` on {info['name']} ({info['cu_count']} CUs) and one CPU thread "
             f"of the same box.  Valid chains, difficulty 0.  Median [min, max] in ms over {REPS} calls after {WARM} "
             "warm-up calls; see the tool's docstring for what each column times.", "",
             "| chains x length | blocks | chains call ms | kernel ms | us per chain (chains call) | "
             "pow_verify_chain loop ms | us per chain (loop) | ref -O2 loop ms | loop / chains call | "
             "ref / chains call |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for n, k, g, kern, lp, c in rows:
        lines.append(f"| {n:,} x {k} | {n * k:,} | {g[0]:.3f} [{g[1]:.3f}, {g[2]:.3f}] | {kern:.3f} | "
                     f"{g[0] * 1e3 / n:.2f} | {lp[0]:.3f} [{lp[1]:.3f}, {lp[2]:.3f}] | {lp[0] * 1e3 / n:.2f} | "
                     f"{c[0]:.3f} [{c[1]:.3f}, {c[2]:.3f}] | {lp[0] / g[0]:.2f}x | {c[0] / g[0]:.2f}x |")
    slower_loop = [f"{n:,} x {k}" for n, k, g, _, lp, _ in rows if g[0] >= lp[0]]
    slower_ref = [f"{n:,} x {k}" for n, k, g, _, _, c in rows if g[0] >= c[0]]
    lines += ["",
              "Against the loop of `pow_verify_chain` calls the batch call "
              + ("is faster at every shape measured." if not slower_loop else
                 "is not faster at: " + ", ".join(slower_loop) + "."),
              "Against the reference's -O2 loop on one CPU thread it "
              + ("is faster at every shape measured." if not slower_ref else
                 "is not faster at: " + ", ".join(slower_ref) + "."), ""]
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(samples, f, indent=1)


if __name__ == "__main__":
    main()
