#!/usr/bin/env python3
"""Cost of the pool's ancestry queries (pow_pool_fork_points, pow_pool_chain) on
one MI355X, against what a caller had to do before them: bring parent and
depth of the whole pool down with pow_pool_read after an add and walk on the
host, or keep a second copy of the tree on the host and walk that.  Pools at
difficulty 0 from tools/pool_cpu.cpp pool_make (a trunk of half the blocks on
one root, the rest as eight chains that fork from the trunk's tip), shuffled.
a is the best tip, b the tip of another of the eight chains: their fork point
is the trunk's tip, about N / 16 steps under either.  For a pool of N blocks:

  first       the first query of a pool that has just been filled in one add:
              the table's allocation, every row over all blocks, the query
  query       pow_pool_fork_points(a, b), one pair, the table up to date
  after add   one block added on the best tip (not timed), then
              pow_pool_fork_points(old best, new best): the table is extended
              by that block inside the call
  4,096 pairs pow_pool_fork_points over 4,096 random pairs, the table up to date
  chain 5     pow_pool_chain(a, 5): the VALIDATION_BLOCKS under the tip
  chain all   pow_pool_chain(a): the whole walk, about 9 N / 16 blocks
  read + walk pow_pool_read of parent and depth for all N blocks, then
              pool_walk_fork(a, b) on the host (tools/pool_cpu.cpp): what the
              header told a caller to do, after every add
  host walk   pool_walk_fork(a, b) alone, on arrays the host already has:
              a caller that keeps a second copy of the tree
  host chain  pool_walk_chain(a) alone, the whole walk

Host clock around every call; kernel ms and launches are pow_get_stats' for
that call.  Median [min, max] of 9 repetitions (or --calls) after 2 warm-up
repetitions; `first` is 3 repetitions, each on a pool of its own.  Every
device answer is held against the host walk's before anything is reported.
Writes the table to profiles/pool_lift/README.md (or --out) and prints it; --json FILE keeps
every timed call of every row.

    python tools/pool_lift_bench.py [--calls 9] [--out FILE] [--json FILE] [--sizes 31,200,4096,65536,1048560]
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

from mpi_blockchain_amd._lib import Block, PoolInfo, check  # noqa: E402
from mpi_blockchain_amd.miner import GpuMiner  # noqa: E402

import index_blocks_bench as ib  # noqa: E402  (cpu_lib: builds and binds tools/pool_cpu.cpp)

REPS, WARM, FIRST_REPS = 9, 2, 3
BS = ctypes.sizeof(Block)
U32P = ctypes.POINTER(ctypes.c_uint32)


stats_of = ib.Calls  # (median, min, max); the calls are kept for --json


def timed(fn, reps):
    """(median, min, max) ms of fn() and what the last call returned."""
    ts, out = [], None
    for rep in range(WARM + reps):
        t0 = time.perf_counter()
        out = fn()
        if rep >= WARM:
            ts.append((time.perf_counter() - t0) * 1e3)
    return stats_of(ts), out


def bind(C):
    P = ctypes.POINTER(Block)
    C.pool_extend.argtypes, C.pool_extend.restype = [P, P, ctypes.c_size_t, ctypes.c_uint32], None
    C.pool_walk_fork.argtypes = [U32P, U32P, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, U32P, U32P]
    C.pool_walk_fork.restype = ctypes.c_uint32
    C.pool_walk_chain.argtypes = [U32P, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_size_t, U32P]
    C.pool_walk_chain.restype = ctypes.c_size_t
    return C


def main():
    global REPS
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pool_lift", "README.md"))
    ap.add_argument("--sizes", default="31,200,4096,65536,1048560")
    ap.add_argument("--calls", type=int, default=REPS)
    ap.add_argument("--json")
    args = ap.parse_args()
    REPS = args.calls
    C = bind(ib.cpu_lib())
    rows = []
    with GpuMiner(0) as m:
        m.warmup()
        dev = m.device_info()
        L = m.L
        for n in (int(s) for s in args.sizes.split(",")):
            arr = (Block * n)()
            C.pool_make(arr, n, 8)
            plain = np.frombuffer(arr, dtype=np.uint8).reshape(n, BS)
            perm = np.random.default_rng(n).permutation(n)
            where = np.empty(n, dtype=np.int64)
            where[perm] = np.arange(n)  # the block made at i stands at where[i]
            raw = np.ascontiguousarray(plain[perm])
            base = (Block * n).from_buffer(raw)
            assert n > 16  # pool_make forks only then
            trunk = n // 2
            tips = (int(where[trunk + (n - trunk) // 8 - 1]), int(where[n - 1]))  # the first and the last chain's tips
            room = n + WARM + REPS + 1

            def filled():
                pool = m.open_pool(0, reserve=room)
                info = PoolInfo()
                assert check(L.pow_pool_add(pool.handle, base, n, ctypes.byref(info)), L) == 1
                return pool, info

            one = lambda v: (ctypes.c_uint32 * 1)(v)  # noqa: E731
            at, ba, bb = one(0), one(0), one(0)

            # first: a pool of its own per repetition
            first_t, first_k = [], []
            for _ in range(FIRST_REPS):
                pool, info = filled()
                a = info.best  # the tip of one of the longest chains
                b = tips[0] if a != tips[0] else tips[1]
                t0 = time.perf_counter()
                rc = L.pow_pool_fork_points(pool.handle, one(a), one(b), 1, at, ba, bb)
                first_t.append((time.perf_counter() - t0) * 1e3)
                check(rc, L)
                s_first = m.stats()
                first_k.append(s_first["kernel_ms"])
                lift = pool.lift_info()
                pool.close()
            pool, info = filled()
            a = info.best
            parent, depth = np.zeros(room, dtype=np.uint32), np.zeros(room, dtype=np.uint32)
            ha, hb = one(0), one(0)

            def query():
                return check(L.pow_pool_fork_points(pool.handle, one(a), one(b), 1, at, ba, bb), L)

            def read_and_walk():
                check(L.pow_pool_read(pool.handle, 0, n, None, parent.ctypes.data_as(U32P), depth.ctypes.data_as(U32P), None), L)
                return C.pool_walk_fork(parent.ctypes.data_as(U32P), depth.ctypes.data_as(U32P), n, a, b, ha, hb)

            def host_walk():
                return C.pool_walk_fork(parent.ctypes.data_as(U32P), depth.ctypes.data_as(U32P), n, a, b, ha, hb)

            query_t, _ = timed(query, REPS)
            s_query = m.stats()
            read_t, want = timed(read_and_walk, REPS)
            walk_t, _ = timed(host_walk, REPS)
            assert (at[0], ba[0], bb[0]) == (want, ha[0], hb[0]), ((at[0], ba[0], bb[0]), (want, ha[0], hb[0]))
            fork = (at[0], ba[0], bb[0])

            rng = np.random.default_rng(n + 1)
            qa, qb = (np.ascontiguousarray(rng.integers(0, n, 4096, dtype=np.uint32)) for _ in range(2))
            many = [np.zeros(4096, dtype=np.uint32) for _ in range(3)]
            many_t, _ = timed(lambda: check(L.pow_pool_fork_points(
                pool.handle, qa.ctypes.data_as(U32P), qb.ctypes.data_as(U32P), 4096, *(x.ctypes.data_as(U32P) for x in many)), L),
                REPS)
            s_many = m.stats()
            for q in range(0, 4096, 64):
                got = C.pool_walk_fork(parent.ctypes.data_as(U32P), depth.ctypes.data_as(U32P), n, int(qa[q]), int(qb[q]), ha, hb)
                assert (int(many[0][q]), int(many[1][q]), int(many[2][q])) == (got, ha[0], hb[0])

            out, host_out = np.zeros(room, dtype=np.uint32), np.zeros(room, dtype=np.uint32)
            n_out = ctypes.c_size_t()
            five_t, _ = timed(lambda: check(L.pow_pool_chain(pool.handle, a, 5, out.ctypes.data_as(U32P), ctypes.byref(n_out)), L),
                              REPS)
            all_t, _ = timed(lambda: check(L.pow_pool_chain(pool.handle, a, n, out.ctypes.data_as(U32P), ctypes.byref(n_out)), L),
                             REPS)
            s_all = m.stats()
            hchain_t, hlen = timed(lambda: C.pool_walk_chain(parent.ctypes.data_as(U32P), n, a, n, host_out.ctypes.data_as(U32P)),
                                   REPS)
            assert n_out.value == hlen == int(depth[a]) and np.array_equal(out[:hlen], host_out[:hlen])

            # after add: every repetition adds one block on the best tip, then asks where the old and the new best part
            add_t, add_k = [], []
            tip_block, size = Block.from_buffer_copy(raw[a].tobytes()), n
            for rep in range(WARM + REPS):
                nxt = (Block * 1)()
                C.pool_extend(ctypes.pointer(tip_block), nxt, 1, 99)
                old = a if rep == 0 else size - 1
                assert check(L.pow_pool_add(pool.handle, nxt, 1, ctypes.byref(info)), L) == 1 and info.best == size
                size, tip_block = size + 1, Block.from_buffer_copy(bytes(nxt[0]))
                t0 = time.perf_counter()
                rc = L.pow_pool_fork_points(pool.handle, one(old), one(info.best), 1, at, ba, bb)
                dt = (time.perf_counter() - t0) * 1e3
                check(rc, L)
                s_add = m.stats()
                assert (at[0], ba[0], bb[0]) == (old, 0, 1) and pool.lift_info()["extended"] == 1
                if rep >= WARM:
                    add_t.append(dt), add_k.append(s_add["kernel_ms"])
            pool.close()
            row = dict(n=n, fork=fork, chain=hlen, first=stats_of(first_t), first_kernel=statistics.median(first_k),
                       first_launches=s_first["launches"], query=query_t, query_kernel=s_query["kernel_ms"],
                       query_launches=s_query["launches"], add=stats_of(add_t), add_kernel=statistics.median(add_k),
                       add_launches=s_add["launches"], many=many_t, many_kernel=s_many["kernel_ms"], five=five_t, all=all_t,
                       all_kernel=s_all["kernel_ms"], read=read_t, walk=walk_t, hchain=hchain_t, lift=lift)
            rows.append(row)
            print(f"{n:,}: first {row['first'][0]:.3f} ms ({row['first_launches']} launches), query {query_t[0]:.3f}, after add "
                  f"{row['add'][0]:.3f} ({row['add_launches']} launches), read + walk {read_t[0]:.3f}, host walk {walk_t[0]:.4f}",
                  flush=True)
            del base, raw, arr, plain

    def cell(x, digits=3):
        return f"{x[0]:.{digits}f} [{x[1]:.{digits}f}, {x[2]:.{digits}f}]"

    lines = ["# pow_pool_fork_points and pow_pool_chain: cost against reading parent[] down and walking on the host", "",
             f"Measured by `tools/pool_lift_bench.py` on {dev['name']} ({dev['cu_count']} CUs).  Median [min, max] in ms over "
             f"{REPS} repetitions after {WARM} warm-up repetitions (`first`: {FIRST_REPS}, each on a pool of its own); see the "
             "tool's docstring for what each column times.", "",
             "| N | fork point: steps back from a, b | first ms | kernel ms | launches | query ms | kernel ms | launches | "
             "after add ms | kernel ms | launches | 4,096 pairs ms | kernel ms | chain 5 ms | chain all ms (blocks) | kernel ms | "
             "read + walk ms | host walk ms | host chain ms | table rows | table bytes |",
             "|" + "---|" * 21]
    for r in rows:
        lines.append(f"| {r['n']:,} | {r['fork'][1]:,}, {r['fork'][2]:,} | {cell(r['first'])} | {r['first_kernel']:.3f} | "
                     f"{r['first_launches']} | {cell(r['query'])} | {r['query_kernel']:.3f} | {r['query_launches']} | "
                     f"{cell(r['add'])} | {r['add_kernel']:.3f} | {r['add_launches']} | {cell(r['many'])} | "
                     f"{r['many_kernel']:.3f} | {cell(r['five'])} | {cell(r['all'])} ({r['chain']:,}) | {r['all_kernel']:.3f} | "
                     f"{cell(r['read'])} | {cell(r['walk'], 4)} | {cell(r['hchain'], 4)} | {r['lift']['rows']} | "
                     f"{r['lift']['bytes']:,} |")
    slower = [f"{r['n']:,}" for r in rows if r["add"][0] >= r["read"][0]]
    lines += ["", "Against pow_pool_read of the whole pool and a host walk, the query after a one-block add "
              + ("is faster at every size measured." if not slower else "is **slower** at N = " + "; ".join(slower) + ".")]
    behind = [f"{r['n']:,}" for r in rows if r["query"][0] >= r["walk"][0]]
    lines += ["Against a host that keeps its own copy of parent and depth and walks it, the device query "
              + ("is faster at every size measured." if not behind else "is **slower** at N = " + "; ".join(behind)
                 + ": one pair is one launch and one bounded wait, the host walk a loop over memory it already has.  "
                   "What that copy costs the host to keep (an O(N) read after every re-rank or prune) is not in its column."),
              "Not measured: a block-major layout of the table; queries from several pools at once.", ""]
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    if args.json:
        ib.write_json(args.json, rows)


if __name__ == "__main__":
    main()
