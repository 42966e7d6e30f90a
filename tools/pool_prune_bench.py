#!/usr/bin/env python3
"""Cost of pow_pool_mark and pow_pool_prune on one MI355X, against what the
library had to do before them to forget the forks that lost: pow_pool_close,
pow_pool_open and one pow_pool_add of every surviving struct.  Pools at
difficulty 0 in the published shape (tools/pool_cpu.cpp pool_make_race: three
rivals per height on a root, every loser a tip), shuffled, sound: the one seed
is the winning tip, so one block per height stays and about two thirds go.
For a pool of N blocks (the largest 3 h + 1 that is at most the size asked for):

  mark        one pow_pool_mark from the winning tip, marks and count down
  prune       one pow_pool_prune from the winning tip, map and info down
  re-add      pow_pool_close, pow_pool_open (reserve = the survivors) and one
              pow_pool_add of the survivors, whose array the host has already
              compacted: what the parent commit's library takes for the same
              pool, in the same process

Every repetition opens a pool and fills it with the N blocks in one add (not
timed), then times the one call, host clock around it; kernel ms and launches
are pow_get_stats' for that call.  Median [min, max] of 9 repetitions (or
--calls) after 2 warm-up repetitions.  The pruned pool is held against the
re-added one (info and all four per-block results) before anything is
reported.  Writes the table to profiles/pool_prune/README.md (or --out) and
prints it.

    python tools/pool_prune_bench.py [--calls 9] [--out FILE] [--json FILE] [--sizes 31,200,4096,65536,1048575]
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

from mpi_blockchain_amd._lib import POOL_NONE, Block, PoolInfo, check  # noqa: E402
from mpi_blockchain_amd.miner import GpuMiner  # noqa: E402

import index_blocks_bench as ib  # noqa: E402  (cpu_lib: builds and binds tools/pool_cpu.cpp)

REPS, WARM = 9, 2
BS = ctypes.sizeof(Block)
U32P = ctypes.POINTER(ctypes.c_uint32)


stats_of = ib.Calls  # (median, min, max); the calls are kept for --json


def device_bytes(cap: int, slots: int) -> int:
    """pow_pool_live_plan's words at that capacity, and the table."""
    return 32 + 96 * cap + 2 * 4 * ((cap + 3) // 4) + 4 * slots


def race_pool(C, heights: int):
    n = 3 * heights + 1
    arr = (Block * n)()
    C.pool_make_race(arr, heights, 3)
    rows = np.frombuffer(arr, dtype=np.uint8).reshape(n, BS)
    perm = np.random.default_rng(n).permutation(n)
    return np.ascontiguousarray(rows[perm])


def filled(m, base, n):
    pool = m.open_pool(0, reserve=n)
    info = PoolInfo()
    assert check(m.L.pow_pool_add(pool.handle, base, n, ctypes.byref(info)), m.L) == 1
    return pool, info


def main():
    global REPS
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pool_prune", "README.md"))
    ap.add_argument("--sizes", default="31,200,4096,65536,1048575")
    ap.add_argument("--calls", type=int, default=REPS)
    ap.add_argument("--json")
    args = ap.parse_args()
    REPS = args.calls
    C = ib.cpu_lib()
    rows = []
    with GpuMiner(0) as m:
        m.warmup()
        dev = m.device_info()
        L = m.L
        for size in (int(s) for s in args.sizes.split(",")):
            heights = (size - 1) // 3
            n = 3 * heights + 1
            t0 = time.perf_counter()
            raw = race_pool(C, heights)
            base = (Block * n).from_buffer(raw)
            print(f"{n:,}: built in {time.perf_counter() - t0:.1f} s", flush=True)
            on, new = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint32)
            n_on, info = ctypes.c_size_t(), PoolInfo()
            mark_t, mark_k, prune_t, prune_k, readd_t, readd_k = [], [], [], [], [], []
            for rep in range(WARM + REPS):
                pool, before = filled(m, base, n)
                tip = (ctypes.c_uint32 * 1)(before.best)
                t0 = time.perf_counter()
                rc = L.pow_pool_mark(pool.handle, tip, 1, 0, 0, on.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n_on))
                dt_mark = (time.perf_counter() - t0) * 1e3
                check(rc, L)
                s_mark = m.stats()
                assert n_on.value == heights + 1 == int(on.sum())
                t0 = time.perf_counter()
                rc = L.pow_pool_prune(pool.handle, tip, 1, 0, 0, new.ctypes.data_as(U32P), ctypes.byref(info))
                dt_prune = (time.perf_counter() - t0) * 1e3
                assert check(rc, L) == 1
                s_prune = m.stats()
                kept = info.size
                assert kept == heights + 1 and np.array_equal(new != POOL_NONE, on.astype(bool))
                pruned = pool.read()
                after = (info.size, info.n_flagged, info.best, info.best_index)
                pool.close()
                # the parent commit's way, from the same filled pool: the survivors' array is the host's own business
                survivors = (Block * kept).from_buffer_copy(np.ascontiguousarray(raw[new != POOL_NONE]).tobytes())
                pool, _ = filled(m, base, n)
                t0 = time.perf_counter()
                pool.close()
                pool = m.open_pool(0, reserve=kept)
                rc = L.pow_pool_add(pool.handle, survivors, kept, ctypes.byref(info))
                dt_readd = (time.perf_counter() - t0) * 1e3
                assert check(rc, L) == 1
                s_readd = m.stats()
                again = pool.read()
                assert after == (info.size, info.n_flagged, info.best, info.best_index)
                for a, b in ((pruned.status, again.status), (pruned.parent, again.parent), (pruned.depth, again.depth),
                             (pruned.n_bad, again.n_bad)):
                    assert a.tobytes() == b.tobytes()
                pool.close()
                if rep >= WARM:
                    mark_t.append(dt_mark), mark_k.append(s_mark["kernel_ms"])
                    prune_t.append(dt_prune), prune_k.append(s_prune["kernel_ms"])
                    readd_t.append(dt_readd), readd_k.append(s_readd["kernel_ms"])
            pool, before = filled(m, base, n)
            tip = (ctypes.c_uint32 * 1)(before.best)
            assert check(L.pow_pool_prune(pool.handle, tip, 1, 0, 0, None, ctypes.byref(info)), L) == 1
            pool.close()
            row = dict(n=n, kept=kept, mark=stats_of(mark_t), mark_kernel=statistics.median(mark_k),
                       mark_launches=s_mark["launches"], prune=stats_of(prune_t), prune_kernel=statistics.median(prune_k),
                       prune_launches=s_prune["launches"], readd=stats_of(readd_t), readd_kernel=statistics.median(readd_k),
                       readd_launches=s_readd["launches"], cap=(before.capacity, info.capacity),
                       slots=(before.slots, info.slots),
                       bytes=(device_bytes(before.capacity, before.slots), device_bytes(info.capacity, info.slots)))
            rows.append(row)
            print(f"{n:,} -> {kept:,}: mark {row['mark'][0]:.3f} ms ({row['mark_launches']} launches, kernel "
                  f"{row['mark_kernel']:.3f}), prune {row['prune'][0]:.3f} ms ({row['prune_launches']} launches, kernel "
                  f"{row['prune_kernel']:.3f}), re-add {row['readd'][0]:.3f} ms ({row['readd_launches']} launches)", flush=True)
            del base, raw, survivors

    def cell(x):
        return f"{x[0]:.3f} [{x[1]:.3f}, {x[2]:.3f}]"

    lines = ["# pow_pool_mark and pow_pool_prune: cost against closing the pool and adding the survivors again", "",
             f"Measured by `tools/pool_prune_bench.py` on {dev['name']} ({dev['cu_count']} CUs).  Median [min, max] in ms over "
             f"{REPS} repetitions after {WARM} warm-up repetitions; see the tool's docstring for what each column times.", "",
             "| N | kept | mark ms | kernel ms | launches | prune ms | kernel ms | launches | close + open + add of the survivors "
             "ms | kernel ms | launches | re-add / prune | capacity before -> after | slots before -> after | device bytes "
             "before -> after |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['n']:,} | {r['kept']:,} | {cell(r['mark'])} | {r['mark_kernel']:.3f} | {r['mark_launches']} | "
                     f"{cell(r['prune'])} | {r['prune_kernel']:.3f} | {r['prune_launches']} | {cell(r['readd'])} | "
                     f"{r['readd_kernel']:.3f} | {r['readd_launches']} | {r['readd'][0] / r['prune'][0]:.2f}x | "
                     f"{r['cap'][0]:,} -> {r['cap'][1]:,} | {r['slots'][0]:,} -> {r['slots'][1]:,} | "
                     f"{r['bytes'][0]:,} -> {r['bytes'][1]:,} |")
    slower = [f"{r['n']:,}" for r in rows if r["prune"][0] >= r["readd"][0]]
    lines += ["", "Against closing the pool and adding the survivors again the prune "
              + ("is faster at every size measured." if not slower else "is **slower** at N = " + "; ".join(slower)
                 + ": it is 6 + ceil(log2 N) launch boundaries, the re-add of a few blocks 3 + ceil(log2 kept)."),
              "The re-add's column leaves out what it costs the host to keep every struct at hand; the prune needs none.",
              "Not measured: the prune against one pow_pool_add of the survivors into a pool that is already open."]
    grown = [f"{r['n']:,} ({r['cap'][0]:,} -> {r['cap'][1]:,})" for r in rows if r["cap"][1] > r["cap"][0]]
    if grown:
        lines += ["A pool opened with a reserve below pow_pool_open's first capacity grows to it: N = " + "; ".join(grown) + "."]
    lines += [""]
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    if args.json:
        ib.write_json(args.json, rows)


if __name__ == "__main__":
    main()
