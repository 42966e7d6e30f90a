#!/usr/bin/env python3
"""Cost of the pool's descendant queries (pow_pool_tips, pow_pool_subtrees,
pow_pool_drop) on one MI355X, against what a caller had to do before them:
bring parent, depth and n_bad of the whole pool down with pow_pool_read and work
on the host with numpy.  Pools at difficulty 0 from tools/pool_cpu.cpp pool_make
(a trunk of half the blocks on one root, the rest as eight chains that fork from
the trunk's tip), shuffled.  For a pool of N blocks:

  tips        pow_pool_tips, every tip (8 of them)
  subtrees 1  pow_pool_subtrees of one root, the first block of a chain that
              lost, no marks, the table up to date
  subtrees 64 the same over 64 roots: that block, the trunk's tip, the root and
              random blocks
  after add   one block added on the best tip (not timed), then subtrees 1: the
              table is extended by that block inside the call
  drop        pow_pool_drop of that losing chain (N / 16 blocks go), each
              repetition on a pool of its own, the table up to date
  read + tips pow_pool_read of parent and n_bad, then the tips by numpy
  read + tree pow_pool_read of parent, depth and n_bad, then the members of the
              one root by numpy doubling, their count, height and fork choice
  prune       the drop's second baseline: pow_pool_prune seeded with the seven
              other tips, which keeps the same blocks; each repetition on a pool
              of its own

Host clock around every call; kernel ms and launches are pow_get_stats' for that
call.  Median [min, max] of 9 repetitions (or --calls) after 2 warm-up
repetitions.  Every device answer is held against the host's before anything is
reported.  Writes the table to profiles/pool_above/README.md (or --out) and
prints it; --json FILE keeps every timed call of every row.

    python tools/pool_above_bench.py [--calls 9] [--out FILE] [--json FILE] [--sizes 31,4096,65536,1048560]
"""
import argparse
import ctypes
import os
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
stats_of = ib.Calls


def timed(fn, reps, before=None):
    """(median, min, max) ms of fn(x), x = before() untimed, and what the last call returned."""
    ts, out = [], None
    for rep in range(WARM + reps):
        x = before() if before else None
        t0 = time.perf_counter()
        out = fn(x) if before else fn()
        if rep >= WARM:
            ts.append((time.perf_counter() - t0) * 1e3)
    return stats_of(ts), out


def host_tips(parent, n_bad, n):
    named = np.zeros(n, dtype=bool)
    named[parent[parent < n]] = True
    return np.flatnonzero(~named)


def host_tree(parent, depth, n_bad, index, n, root):
    """(size, height, best) of root's subtree: the members by doubling along parent."""
    hit = np.arange(n) == root
    jump = parent.astype(np.int64)
    while True:
        live = jump < n
        if not live.any():
            break
        at = np.where(live, jump, 0)
        hit = hit | (live & hit[at])
        jump = np.where(live, jump[at], jump)
    pos = np.flatnonzero(hit & (n_bad == 0))
    best = int(pos[np.argmax(index[pos])]) if len(pos) else POOL_NONE
    return int(hit.sum()), int(depth[hit].max()) - int(depth[root]), best, hit


def main():
    global REPS
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pool_above", "README.md"))
    ap.add_argument("--sizes", default="31,4096,65536,1048560")
    ap.add_argument("--calls", type=int, default=REPS)
    ap.add_argument("--json")
    args = ap.parse_args()
    REPS = args.calls
    C = ib.cpu_lib()
    P = ctypes.POINTER(Block)
    C.pool_extend.argtypes, C.pool_extend.restype = [P, P, ctypes.c_size_t, ctypes.c_uint32], None
    rows = []
    with GpuMiner(0) as m:
        m.warmup()
        dev = m.device_info()
        L = m.L
        for n in (int(s) for s in args.sizes.split(",")):
            assert n > 16  # pool_make forks only then
            arr = (Block * n)()
            C.pool_make(arr, n, 8)
            plain = np.frombuffer(arr, dtype=np.uint8).reshape(n, BS)
            perm = np.random.default_rng(n).permutation(n)
            where = np.empty(n, dtype=np.int64)
            where[perm] = np.arange(n)  # the block made at i stands at where[i]
            raw = np.ascontiguousarray(plain[perm])
            base = (Block * n).from_buffer(raw)
            index = np.frombuffer(raw, dtype=np.uint32).reshape(n, BS // 4)[:, Block.index.offset // 4].copy()
            trunk, spans, at = n // 2, [], n // 2
            for b in range(8):  # pool_make's eight chains, in the order it made them
                spans.append((at, at + (n - at) // (8 - b)))
                at = spans[-1][1]
            room = n + WARM + REPS + 1

            def filled(query=True):
                pool = m.open_pool(0, reserve=room)
                info = PoolInfo()
                assert check(L.pow_pool_add(pool.handle, base, n, ctypes.byref(info)), L) == 1
                if query:  # the table up to date
                    pool.subtrees([0])
                return pool, info

            pool, info = filled()
            best = info.best
            firsts, ends = [int(where[a]) for a, _ in spans], [int(where[b - 1]) for _, b in spans]
            lost = next(c for c in range(8) if ends[c] != best)
            root = firsts[lost]
            rng = np.random.default_rng(n + 1)
            many = np.ascontiguousarray(np.concatenate([[root, int(where[trunk - 1]), int(where[0])],
                                                        rng.integers(0, n, 61)]).astype(np.uint32))
            one = (ctypes.c_uint32 * 1)(root)
            parent, depth, n_bad = (np.zeros(room, dtype=np.uint32) for _ in range(3))
            out = np.zeros(n, dtype=np.uint32)
            n_out = ctypes.c_size_t()
            res = [np.zeros(64, dtype=np.uint32) for _ in range(4)]
            ptr = [x.ctypes.data_as(U32P) for x in res]

            tips_t, _ = timed(lambda: check(L.pow_pool_tips(pool.handle, 0, out.ctypes.data_as(U32P), n, ctypes.byref(n_out)), L), REPS)
            s_tips = m.stats()
            one_t, _ = timed(lambda: check(L.pow_pool_subtrees(pool.handle, one, 1, *ptr, None, None), L), REPS)
            s_one = m.stats()
            got_one = tuple(int(x[0]) for x in res[:3])
            many_t, _ = timed(lambda: check(L.pow_pool_subtrees(pool.handle, many.ctypes.data_as(U32P), 64, *ptr, None, None), L), REPS)
            s_many = m.stats()

            def read_tips():
                check(L.pow_pool_read(pool.handle, 0, n, None, parent.ctypes.data_as(U32P), None, n_bad.ctypes.data_as(U32P)), L)
                return host_tips(parent[:n], n_bad[:n], n)

            def read_tree():
                check(L.pow_pool_read(pool.handle, 0, n, None, parent.ctypes.data_as(U32P), depth.ctypes.data_as(U32P),
                                      n_bad.ctypes.data_as(U32P)), L)
                return host_tree(parent[:n], depth[:n], n_bad[:n], index, n, root)

            rtips_t, want_tips = timed(read_tips, REPS)
            rtree_t, want_tree = timed(read_tree, REPS)
            assert n_out.value == len(want_tips) == 8 and np.array_equal(out[:8], want_tips)
            assert got_one == want_tree[:3] and want_tree[0] == spans[lost][1] - spans[lost][0], (got_one, want_tree[:3])
            keep_tips = (ctypes.c_uint32 * 7)(*[e for c, e in enumerate(ends) if c != lost])

            # after add: every repetition adds one block on the best tip, then asks for the losing chain again
            add_t = []
            tip_block, size = Block.from_buffer_copy(raw[best].tobytes()), n
            for rep in range(WARM + REPS):
                nxt = (Block * 1)()
                C.pool_extend(ctypes.pointer(tip_block), nxt, 1, 99)
                assert check(L.pow_pool_add(pool.handle, nxt, 1, ctypes.byref(info)), L) == 1 and info.best == size
                size, tip_block = size + 1, Block.from_buffer_copy(bytes(nxt[0]))
                t0 = time.perf_counter()
                rc = L.pow_pool_subtrees(pool.handle, one, 1, *ptr, None, None)
                dt = (time.perf_counter() - t0) * 1e3
                check(rc, L)
                s_add = m.stats()
                assert tuple(int(x[0]) for x in res[:3]) == got_one and pool.lift_info()["extended"] == 1
                if rep >= WARM:
                    add_t.append(dt)
            pool.close()

            # drop and its second baseline: destructive, so every repetition has a pool of its own
            new = np.zeros(n, dtype=np.uint32)
            done = []

            def drop(pool):
                rc = L.pow_pool_drop(pool.handle, one, 1, new.ctypes.data_as(U32P), ctypes.byref(info))
                done.append((pool, m.stats(), new.copy(), info.size))
                return check(rc, L)

            def prune(pool):
                rc = L.pow_pool_prune(pool.handle, keep_tips, 7, 0, 0, new.ctypes.data_as(U32P), ctypes.byref(info))
                done.append((pool, m.stats(), new.copy(), info.size))
                return check(rc, L)

            drop_t, _ = timed(drop, REPS, before=lambda: filled()[0])
            s_drop, map_drop, left = done[-1][1:]
            for p, *_ in done:
                p.close()
            done.clear()
            prune_t, _ = timed(prune, REPS, before=lambda: filled(False)[0])
            s_prune, map_prune, left_prune = done[-1][1:]
            for p, *_ in done:
                p.close()
            done.clear()
            assert left == left_prune == n - want_tree[0] and np.array_equal(map_drop, map_prune)
            assert np.array_equal(map_drop == POOL_NONE, want_tree[3])
            row = dict(n=n, gone=want_tree[0], height=want_tree[1], tips=tips_t, tips_kernel=s_tips["kernel_ms"],
                       tips_launches=s_tips["launches"], one=one_t, one_kernel=s_one["kernel_ms"], one_launches=s_one["launches"],
                       many=many_t, many_kernel=s_many["kernel_ms"], add=stats_of(add_t), add_launches=s_add["launches"],
                       drop=drop_t, drop_kernel=s_drop["kernel_ms"], drop_launches=s_drop["launches"], read_tips=rtips_t,
                       read_tree=rtree_t, prune=prune_t, prune_kernel=s_prune["kernel_ms"], prune_launches=s_prune["launches"])
            rows.append(row)
            print(f"{n:,}: tips {tips_t[0]:.3f} ms, subtrees 1 {one_t[0]:.3f}, 64 {many_t[0]:.3f}, after add {row['add'][0]:.3f}, "
                  f"drop {drop_t[0]:.3f} ({row['drop_launches']} launches); read + tips {rtips_t[0]:.3f}, read + tree "
                  f"{rtree_t[0]:.3f}, prune {prune_t[0]:.3f}", flush=True)
            del base, raw, arr, plain

    def cell(x, digits=3):
        return f"{x[0]:.{digits}f} [{x[1]:.{digits}f}, {x[2]:.{digits}f}]"

    lines = ["# pow_pool_tips, pow_pool_subtrees and pow_pool_drop: cost against reading the pool down and numpy on the host", "",
             f"Measured by `tools/pool_above_bench.py` on {dev['name']} ({dev['cu_count']} CUs).  Median [min, max] in ms over "
             f"{REPS} repetitions after {WARM} warm-up repetitions; see the tool's docstring for what each column times.", "",
             "| N | blocks dropped | tips ms | kernel ms | launches | subtrees 1 ms | kernel ms | launches | subtrees 64 ms | kernel ms | "
             "after add ms | launches | drop ms | kernel ms | launches | read + tips ms | read + tree ms | prune ms | kernel ms | "
             "launches |",
             "|" + "---|" * 20]
    for r in rows:
        lines.append(f"| {r['n']:,} | {r['gone']:,} | {cell(r['tips'])} | {r['tips_kernel']:.3f} | {r['tips_launches']} | "
                     f"{cell(r['one'])} | {r['one_kernel']:.3f} | {r['one_launches']} | {cell(r['many'])} | {r['many_kernel']:.3f} | "
                     f"{cell(r['add'])} | {r['add_launches']} | {cell(r['drop'])} | {r['drop_kernel']:.3f} | {r['drop_launches']} | "
                     f"{cell(r['read_tips'])} | {cell(r['read_tree'])} | {cell(r['prune'])} | {r['prune_kernel']:.3f} | "
                     f"{r['prune_launches']} |")
    for name, col, base_col, text in (("pow_pool_tips", "tips", "read_tips", "pow_pool_read and numpy"),
                                      ("pow_pool_subtrees after a one-block add", "add", "read_tree", "pow_pool_read and numpy"),
                                      ("pow_pool_drop", "drop", "prune", "pow_pool_prune seeded with the other tips")):
        slower = [f"{r['n']:,}" for r in rows if r[col][0] >= r[base_col][0]]
        lines += ["", f"Against {text}, {name} "
                  + ("is faster at every size measured." if not slower else "is **slower** at N = " + "; ".join(slower) + ".")]
    lines += ["", "The prune's seeds (the tips of what is to stay) are given to it here; a caller that has to find them first "
              "pays for `read + tips` or a pow_pool_tips call on top.  Not measured: more than one pool at a time.", ""]
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    if args.json:
        ib.write_json(args.json, rows)


if __name__ == "__main__":
    main()
