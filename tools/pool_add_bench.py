#!/usr/bin/env python3
"""Cost of one arrival at a pool that stays on the GPU (pow_pool_add) on one
MI355X, against what the parent commit must do for the same answer
(pow_index_blocks over all N + 1 blocks) and against the reference's way on
one CPU thread of the same box.  Pools at difficulty 0 (tools/pool_cpu.cpp
makes them: a trunk of N / 2 blocks and 8 branches from its tip), shuffled,
sound.  For a pool of N blocks:

  add 1       one pow_pool_add of one block on a tip: the fast path
  re-rank     one pow_pool_add of one block whose child arrived before it: the
              add adopts the orphan and ranks the whole pool again
  add 5       one pow_pool_add of a run of 5 blocks on a tip (a migrated run)
  index call  pow_index_blocks over the N + 1 blocks
  ref -O2     tools/pool_cpu.cpp pool_ref_add, one CPU thread: the std::map
              insert and the sanity_test walk from the new tip with
              block_to_hash per block (of 1 block, and of the run of 5)

Every repetition opens a pool, fills it with the N blocks in one add (not
timed) and times the one add, host clock around the call; kernel ms is
pow_get_stats' for that add.  Median [min, max] of 9 repetitions (or --calls)
after 2 warm-up repetitions.  Where N + the arrival would pass
POW_POOL_MAX_BLOCKS, the re-rank's and the run's pools are that much smaller
(pools of their own, built the same way).  Writes the table to
profiles/pool_stream/README.md (or --out) and prints it; --json FILE keeps
every timed call of every row.

    python tools/pool_add_bench.py [--calls 9] [--out FILE] [--json FILE] [--sizes 31,200,4096,65536,1048575]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

from mpi_blockchain_amd._lib import POOL_MAX_BLOCKS, Block, PoolInfo, check  # noqa: E402
from mpi_blockchain_amd.miner import GpuMiner  # noqa: E402

import index_blocks_bench as ib  # noqa: E402  (cpu_lib: builds and binds tools/pool_cpu.cpp)

REPS, WARM = 9, 2
BS = ctypes.sizeof(Block)


def cpu_lib():
    C = ib.cpu_lib()
    P = ctypes.POINTER(Block)
    C.pool_extend.argtypes, C.pool_extend.restype = [P, P, ctypes.c_size_t, ctypes.c_uint32], None
    C.pool_ref_new.argtypes, C.pool_ref_new.restype = [P, ctypes.c_size_t], ctypes.c_void_p
    C.pool_ref_free.argtypes, C.pool_ref_free.restype = [ctypes.c_void_p], None
    C.pool_ref_add.argtypes = [ctypes.c_void_p, P, ctypes.c_size_t, ctypes.c_uint, ctypes.POINTER(ctypes.c_uint64)]
    C.pool_ref_add.restype = ctypes.c_int
    C.pool_ref_drop.argtypes, C.pool_ref_drop.restype = [ctypes.c_void_p, P, ctypes.c_size_t], None
    return C


stats_of = ib.Calls  # (median, min, max); the calls are kept for --json


def shuffled_pool(C, n):
    arr = (Block * n)()
    C.pool_make(arr, n, 8)
    rows = np.frombuffer(arr, dtype=np.uint8).reshape(n, BS)
    perm = np.random.default_rng(n).permutation(n)
    return (Block * n).from_buffer_copy(np.ascontiguousarray(rows[perm]).tobytes())


def timed_adds(m, base, n, before, arrival, want):
    """REPS timed pow_pool_add calls of `arrival`, each into a pool just filled
    with base[:n] (and `before`, if any); want = (adopted, reranked)."""
    L = m.L
    info, ts, kernel, launches = PoolInfo(), [], [], 0
    k = len(arrival)
    for rep in range(WARM + REPS):
        with m.open_pool(0, reserve=n + len(before or ()) + k) as pool:
            assert check(L.pow_pool_add(pool.handle, base, n, None), L) == 1
            if before is not None:
                assert check(L.pow_pool_add(pool.handle, before, len(before), None), L) == 0  # an orphan
            t0 = time.perf_counter()
            rc = L.pow_pool_add(pool.handle, arrival, k, ctypes.byref(info))
            dt = (time.perf_counter() - t0) * 1e3
            assert check(rc, L) == 1 and (info.adopted, info.reranked) == want and info.rehashed == 0, \
                (rc, info.adopted, info.reranked, info.rehashed)
            if rep >= WARM:
                ts.append(dt)
                s = m.stats()
                kernel.append(s["kernel_ms"])
                launches = s["launches"]
            final = (info.size, info.best, info.best_index, info.capacity, info.slots)
    return stats_of(ts), statistics.median(kernel), launches, final


def main():
    global REPS
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pool_stream", "README.md"))
    ap.add_argument("--sizes", default="31,200,4096,65536,1048575")
    ap.add_argument("--calls", type=int, default=REPS)
    ap.add_argument("--json")
    args = ap.parse_args()
    REPS = args.calls
    C = cpu_lib()
    rows, memory = [], None
    with GpuMiner(0) as m:
        m.warmup()
        dev = m.device_info()
        L, ctx = m.L, m.ctx
        for size in (int(s) for s in args.sizes.split(",")):
            room = POOL_MAX_BLOCKS - size
            n1, n2, n5 = size - max(0, 1 - room), size - max(0, 2 - room), size - max(0, 5 - room)
            built = {}

            def prepare(n):
                """A shuffled pool of n blocks, and a run of 5 on one of its tips."""
                if n not in built:
                    built.clear()  # one pool of 2^20 blocks at a time
                    t0 = time.perf_counter()
                    base = shuffled_pool(C, n)
                    tip = int(np.argmax(np.frombuffer(base, dtype=np.uint32).reshape(n, BS // 4)[:, 0]))
                    run = (Block * 5)()
                    C.pool_extend(ctypes.byref(base[tip]), run, 5, 99)
                    built[n] = base, (Block * 1)(run[0]), (Block * 1)(run[1]), run
                    print(f"{n:,}: built in {time.perf_counter() - t0:.1f} s", flush=True)
                return built[n]

            base, one, child, run = prepare(n5)
            five = timed_adds(m, base, n5, None, run, (0, 0))
            base, one, child, run = prepare(n2)
            rerank = timed_adds(m, base, n2, child, one, (1, 1))
            base, one, child, run = prepare(n1)
            fast = timed_adds(m, base, n1, None, one, (0, 0))

            # the same answer from one pow_index_blocks call over the n1 + 1 blocks
            raw = np.empty((n1 + 1) * BS, dtype=np.uint8)
            raw[:n1 * BS] = np.frombuffer(base, dtype=np.uint8)[:n1 * BS]
            raw[n1 * BS:] = np.frombuffer(one, dtype=np.uint8)
            both = (Block * (n1 + 1)).from_buffer(raw)
            best, ts, kern = ctypes.c_size_t(), [], []
            for rep in range(WARM + REPS):
                t0 = time.perf_counter()
                rc = L.pow_index_blocks(ctx, both, n1 + 1, 0, None, None, None, None, ctypes.byref(best))
                dt = (time.perf_counter() - t0) * 1e3
                assert check(rc, L) == 1
                if rep >= WARM:
                    ts.append(dt)
                    kern.append(m.stats()["kernel_ms"])
            index = stats_of(ts), statistics.median(kern), m.stats()["launches"]
            assert fast[3][:3] == (n1 + 1, best.value, both[best.value].index), (fast[3], best.value)
            del both

            # the reference's way: node_blocks kept, the arrival inserted and the walk from the new tip
            ref = []
            handle = C.pool_ref_new(base, n1)
            walked = ctypes.c_uint64()
            for arrival, k in ((one, 1), (run, 5)):
                ts = []
                for rep in range(WARM + REPS):
                    t0 = time.perf_counter()
                    ok = C.pool_ref_add(handle, arrival, k, 0, ctypes.byref(walked))
                    dt = (time.perf_counter() - t0) * 1e3
                    C.pool_ref_drop(handle, arrival, k)
                    assert ok == 1
                    if rep >= WARM:
                        ts.append(dt)
                ref.append((stats_of(ts), walked.value))
            C.pool_ref_free(handle)
            rows.append((size, n1, n2, n5, fast, rerank, five, index, ref))
            print(f"{size:,}: add 1 {fast[0][0]:.3f} ms ({fast[2]} launches, kernel {fast[1]:.3f}), re-rank "
                  f"{rerank[0][0]:.3f} ms ({rerank[2]} launches), add 5 {five[0][0]:.3f} ms ({five[2]} launches), index call "
                  f"{index[0][0]:.3f} ms, ref {ref[0][0][0]:.3f} ms ({ref[0][1]:,} blocks walked)", flush=True)
            cap, slots = fast[3][3], fast[3][4]
            memory = (n1 + 1, cap, slots, 32 + 96 * cap + 2 * 4 * ((cap + 3) // 4) + 4 * slots)
            del base

    def cell(x):
        return f"{x[0]:.3f} [{x[1]:.3f}, {x[2]:.3f}]"

    lines = ["# pow_pool_add: cost per arrival", "",
             f"Measured by `tools/pool_add_bench.py` on {dev['name']} ({dev['cu_count']} CUs) and one CPU thread of the same box.  "
             f"Median [min, max] in ms over {REPS} repetitions after {WARM} warm-up repetitions; see the tool's docstring for "
             "what each column times.", "",
             "| N | add 1 ms | kernel ms | launches | re-rank add ms | kernel ms | launches | add 5 ms | launches | "
             "pow_index_blocks(N + 1) ms | ref -O2, 1 block ms | blocks walked | ref -O2, 5 blocks ms | index call / add 1 | "
             "ref / add 1 |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for size, n1, n2, n5, fast, rerank, five, index, ref in rows:
        note = "" if (n1, n2, n5) == (size, size, size) else f" (re-rank at {n2:,}, add 5 at {n5:,})"
        lines.append(f"| {n1:,}{note} | {cell(fast[0])} | {fast[1]:.3f} | {fast[2]} | {cell(rerank[0])} | {rerank[1]:.3f} | "
                     f"{rerank[2]} | {cell(five[0])} | {five[2]} | {cell(index[0])} | {cell(ref[0][0])} | {ref[0][1]:,} | "
                     f"{cell(ref[1][0])} | {index[0][0] / fast[0][0]:.2f}x | {ref[0][0][0] / fast[0][0]:.2f}x |")
    if memory:
        lines += ["", f"Device memory of the last pool ({memory[0]:,} blocks, capacity {memory[1]:,}, {memory[2]:,} slots): "
                  f"{memory[3] / 1e6:.1f} MB of arrays and table, the context's tile staging buffer apart."]
    slower = [f"{r[1]:,}" for r in rows if r[4][0][0] >= r[8][0][0][0]]
    lines += ["", "Against the reference's map insert and walk on one CPU thread the add of one block "
              + ("is faster at every size measured." if not slower else "is **not faster** at N = " + "; ".join(slower) + "."), ""]
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    if args.json:  # fast, rerank, five: (calls, kernel ms, launches, (size, best, best_index, capacity, slots))
        ib.write_json(args.json, rows, ("size", "n1", "n2", "n5", "fast", "rerank", "five", "index", "ref"))


if __name__ == "__main__":
    main()
