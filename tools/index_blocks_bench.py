#!/usr/bin/env python3
"""Cost of "which blocks of this pool hang together, which chains are sound and
which tip wins?" on one MI355X and on the same box's CPU.  Pools at difficulty
0 (tools/pool_cpu.cpp makes them), shuffled:

  race 3x10   the published shape as a pool: 3 rivals x 10 heights on a root,
              every loser a tip (31 blocks, 21 tips)
  n blocks    a trunk of n / 2 blocks and 8 branches from its tip (8 tips);
              16 blocks or fewer: one chain

  index call  pow_index_blocks over the pool, host clock around the call
  kernel      kernel_ms of pow_get_stats for that call (HIP events)
  ref -O2     tools/pool_cpu.cpp pool_ref_audit, one CPU thread: a std::map
              keyed on the stored text, then the sanity_test walk from every
              tip with block_to_hash per block (shared prefixes hashed once
              per tip, as the reference would)
  today       tools/pool_cpu.cpp pool_extract (the map, the tips, every tip's
              chain copied out) and then ONE pow_verify_chains call over them

Median [min, max] of 9 calls (or --calls) after 2 warm-up calls.  Writes the
table to profiles/index_blocks/README.md (or --out) and prints it; --json FILE keeps
every timed call of every row.

    python tools/index_blocks_bench.py [--calls 9] [--out FILE] [--json FILE] [--device-only] [--shapes 5,16,race,200,4096,65536,1048576]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from mpi_blockchain_amd._lib import Block, check  # noqa: E402
from mpi_blockchain_amd.miner import GpuMiner  # noqa: E402

SRC = os.path.join(ROOT, "tools", "pool_cpu.cpp")
LIB = os.path.join(ROOT, "tools", "libpool_cpu.so")
REPS, WARM = 9, 2
SIZE_MAX = ctypes.c_size_t(-1).value


def cpu_lib():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < os.path.getmtime(SRC):
        subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-I", os.path.join(ROOT, "include"), SRC,
                        "-o", LIB], check=True)
    C = ctypes.CDLL(LIB)
    P, szp = ctypes.POINTER(Block), ctypes.POINTER(ctypes.c_size_t)
    C.pool_make.argtypes, C.pool_make.restype = [P, ctypes.c_size_t, ctypes.c_size_t], None
    C.pool_make_race.argtypes, C.pool_make_race.restype = [P, ctypes.c_size_t, ctypes.c_size_t], None
    C.pool_ref_audit.argtypes = [P, ctypes.c_size_t, ctypes.c_uint, szp, szp, ctypes.POINTER(ctypes.c_uint64)]
    C.pool_ref_audit.restype = ctypes.c_size_t
    C.pool_extract.argtypes = [P, ctypes.c_size_t, P, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32), szp]
    C.pool_extract.restype = ctypes.c_size_t
    return C


class Calls(tuple):
    """(median, min, max) ms of timed calls; .ms keeps the calls themselves for --json."""

    def __new__(cls, ts):
        self = super().__new__(cls, (statistics.median(ts), min(ts), max(ts)))
        self.ms = list(ts)
        return self


def write_json(path, rows, names=None):
    """--json FILE (this tool and the pool tools): every row as it was measured,
    a timed column as {"ms": its calls}, so that a script can take medians and
    interquartile ranges; names = the fields of a row that is a tuple."""
    def plain(v):
        if isinstance(v, Calls):
            return {"ms": v.ms}
        if isinstance(v, dict):
            return {k: plain(x) for k, x in v.items()}
        if isinstance(v, (tuple, list)):
            return [plain(x) for x in v]
        return v.item() if isinstance(v, np.generic) else v

    with open(path, "w") as f:
        json.dump([plain(dict(zip(names, r)) if names else r) for r in rows], f, indent=1, default=str)


def median_ms(fn):
    for _ in range(WARM):
        fn()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return Calls(ts)


def make_pool(C, shape: str):
    """(name, shuffled pool, blocks, tips, blocks of all tips' chains)."""
    if shape == "race":
        n, tips = 31, 21
        arr = (Block * n)()
        C.pool_make_race(arr, 10, 3)
        name, walked = "race 3 x 10", sum(h + 1 for h in range(1, 11)) * 2 + 11  # two losers per height, and the last winner
    else:
        n = int(shape)
        arr = (Block * n)()
        C.pool_make(arr, n, 8)
        if n > 16:
            name, tips, walked = f"{n:,}", 8, 8 * (n // 2) + (n - n // 2)
        else:  # too few blocks to fork eight times: one chain
            name, tips, walked = f"{n:,} (one chain)", 1, n
    rows = np.frombuffer(arr, dtype=np.uint8).reshape(n, ctypes.sizeof(Block))
    perm = np.random.default_rng(n).permutation(n)
    return name, (Block * n).from_buffer_copy(np.ascontiguousarray(rows[perm]).tobytes()), n, tips, walked


def main():
    global REPS
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_blocks", "README.md"))
    ap.add_argument("--shapes", default="5,16,race,200,4096,65536,1048576")
    ap.add_argument("--calls", type=int, default=REPS)
    ap.add_argument("--json")
    ap.add_argument("--device-only", action="store_true",
                    help="time the index call alone: the two CPU columns (19 s and 15 s a call at 2^20 blocks) read nan")
    args = ap.parse_args()
    REPS = args.calls
    C = cpu_lib()
    rows, tops = [], []
    with GpuMiner(0) as m:
        m.warmup()
        info = m.device_info()
        L, ctx = m.L, m.ctx
        for shape in args.shapes.split(","):
            t0 = time.perf_counter()
            name, pool, n, tips, walked = make_pool(C, shape)
            print(f"{name}: built in {time.perf_counter() - t0:.1f} s", flush=True)
            best, kernel = ctypes.c_size_t(), []

            def index_call():
                rc = check(L.pow_index_blocks(ctx, pool, n, 0, None, None, None, None, ctypes.byref(best)), L)
                assert rc == 1 and best.value != SIZE_MAX
                kernel.append(m.stats()["kernel_ms"])

            g = median_ms(index_call)
            kern = statistics.median(kernel[-REPS:])
            launches = m.stats()["launches"]
            top = pool[best.value].index
            assert top == max(b.index for b in pool) if n <= 4096 else True

            n_tips, ref_best, hashed = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_uint64()

            def ref_call():
                sound = C.pool_ref_audit(pool, n, 0, ctypes.byref(n_tips), ctypes.byref(ref_best), ctypes.byref(hashed))
                assert sound == n_tips.value == tips and hashed.value == walked, (sound, n_tips.value, hashed.value, walked)

            c = Calls([float("nan")]) if args.device_only else median_ms(ref_call)
            assert args.device_only or pool[ref_best.value].index == top

            out = (Block * walked)()
            lengths = (ctypes.c_uint32 * tips)()
            n_chains, vbest = ctypes.c_size_t(), ctypes.c_size_t()

            def today_call():
                total = C.pool_extract(pool, n, out, walked, lengths, ctypes.byref(n_chains))
                assert total == walked and n_chains.value == tips
                rc = check(L.pow_verify_chains(ctx, out, lengths, tips, 0, None, None, None, ctypes.byref(vbest)), L)
                assert rc == 1

            t = Calls([float("nan")]) if args.device_only else median_ms(today_call)
            assert args.device_only or out[sum(lengths[:vbest.value])].index == top
            rows.append((name, n, tips, walked, launches, g, kern, c, t))
            tops.append(top)
            print(f"{name}: index call {g[0]:.3f} ms (kernel {kern:.3f}, {launches} launches), ref -O2 {c[0]:.3f} ms, "
                  f"today {t[0]:.3f} ms", flush=True)
            del out
    lines = ["# pow_index_blocks: cost per call", "",
             f"Measured by `tools/index_blocks_bench.py` on {info['name']} ({info['cu_count']} CUs) and one CPU thread of the "
             f"same box.  Sound pools at difficulty 0, shuffled.  Median [min, max] in ms over {REPS} calls after {WARM} "
             "warm-up calls; see the tool's docstring for the shapes and for what each column times.", "",
             "| pool | blocks | tips | blocks of all tips' chains | launches | index call ms | kernel ms | ref -O2 ms | "
             "extract + pow_verify_chains ms | ref / index call | today / index call |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for name, n, tips, walked, launches, g, kern, c, t in rows:
        lines.append(f"| {name} | {n:,} | {tips} | {walked:,} | {launches} | {g[0]:.3f} [{g[1]:.3f}, {g[2]:.3f}] | {kern:.3f} | "
                     f"{c[0]:.3f} [{c[1]:.3f}, {c[2]:.3f}] | {t[0]:.3f} [{t[1]:.3f}, {t[2]:.3f}] | {c[0] / g[0]:.2f}x | "
                     f"{t[0] / g[0]:.2f}x |")
    slower_ref = [r[0] for r in rows if r[5][0] >= r[7][0]]
    slower_today = [r[0] for r in rows if r[5][0] >= r[8][0]]
    lines += ["",
              "Against the reference's way on one CPU thread the call "
              + ("is faster at every shape measured." if not slower_ref else "is not faster at: " + "; ".join(slower_ref) + "."),
              "Against host extraction and one `pow_verify_chains` call it "
              + ("is faster at every shape measured." if not slower_today else
                 "is not faster at: " + "; ".join(slower_today) + "."), ""]
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    if args.json:
        write_json(args.json, [r + (top,) for r, top in zip(rows, tops)],
                   ("pool", "blocks", "tips", "walked", "launches", "index_call", "kernel_ms", "ref", "today", "best_index"))


if __name__ == "__main__":
    main()
