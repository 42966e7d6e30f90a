#!/usr/bin/env python3
"""Wall time per height of a race of R rival miners, three ways, on one GPU in
one run:

  (a) fused       one pow_mine_race call, K6 forced at every d (test library,
                  POW_RACE_FUSED_MAX=32)
  (b) host-loop   one pow_mine_race call on the library's host loop (test
                  library, POW_RACE_FUSED_MAX=-1): per height refresh + pow_mine
                  rival by rival, each below the best counter so far
  (c) batch-loop  the loop of examples/mine_race.c from C against the shipped
                  library: per height one pow_mine_batch call, which finds every
                  loser's solution too

All run the same race (tools/mine_race_bench.c) at R = 3 and 64 over `--heights`
heights and the window 2^(d + 7), what the examples pass.  Every value is the
median of `--calls` (>= 7) calls after pow_warmup and one discarded call, with
the interquartile range beside it; each way runs in its own process.  The
outputs of the ways are compared by checksum (every byte, winner and counter),
and each passes pow_verify_chain.  The published 3-node shape (3 rivals, 10
heights, d = 18, window 2^32) follows, then a row of K6's POW_RACE_LANES_LOG2
{0, 2, 4} at d = 13 and 19.

The rule for POW_RACE_FUSED_MAX_D (csrc/pow_ctx.h) is applied to the result: the
largest measured d at which (a)'s median is below (b)'s by more than the two
interquartile ranges combined, at both R; -1 if there is none.

    python tools/mine_race_bench.py [--calls 9] [--heights 8] [--out FILE.json]

Each measurement is its own process under a time limit; the first failure ends
the run.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mpi_blockchain_amd")
DS = [9, 13, 17, 19, 21, 23]
RS = [3, 64]
WAYS = {"fused": ("pow_gpu_test", "race", {"POW_RACE_FUSED_MAX": "32"}),
        "host-loop": ("pow_gpu_test", "race", {"POW_RACE_FUSED_MAX": "-1"}),
        "batch-loop": ("pow_gpu", "batch", {})}


def compile_bench(td: str, lib: str) -> str:
    exe = os.path.join(td, "mine_race_bench_" + lib)
    subprocess.run(["gcc", "-std=c11", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "mine_race_bench.c"), "-L", PKG, "-l" + lib, f"-Wl,-rpath,{PKG}",
                    "-o", exe], check=True)
    return exe


def quartiles(xs):
    q = statistics.quantiles(xs, n=4, method="inclusive")
    return statistics.median(xs), q[2] - q[0]


def measure(exes, way: str, d: int, wlog: int, heights: int, rs, calls: int, extra_env=None) -> dict:
    """One process: every R of `rs` at (d, window).  {R: row}."""
    lib, mode, env = WAYS[way]
    p = subprocess.run(["timeout", "-k", "10", "300", exes[lib], mode, str(d), str(wlog), str(calls), str(heights),
                        *map(str, rs)], capture_output=True, text=True, env={**os.environ, **env, **(extra_env or {})})
    if p.returncode != 0:
        sys.exit(f"{way} d={d} window=2^{wlog}: exit {p.returncode}\n{p.stdout}{p.stderr}")
    rows = {}
    for line in p.stdout.strip().splitlines():
        r = json.loads(line)
        assert r["valid"] == 1, f"{way} d={d} R={r['rivals']}: the mined chain does not pass pow_verify_chain"
        med, iqr = quartiles(r["ms"])
        R = r["rivals"]
        rows[R] = {"way": way, "d": d, "window_log2": wlog, "rivals": R, "heights": heights, "checksum": r["checksum"],
                   "call_ms": med, "call_ms_iqr": iqr, "us_per_height": 1e3 * med / heights,
                   "us_per_height_iqr": 1e3 * iqr / heights, "kernel_ms": statistics.median(r["kernel_ms"]),
                   "launches": int(statistics.median(r["launches"])), "trials": int(statistics.median(r["trials"])),
                   "pairs_needed": r["pairs_needed"], "samples_ms": r["ms"]}
    assert sorted(rows) == sorted(rs)
    return rows


def wins(f: dict, c: dict) -> bool:
    return c["call_ms"] - f["call_ms"] > c["call_ms_iqr"] + f["call_ms_iqr"]


def line(r: dict) -> str:
    return (f"{r['us_per_height']:.1f} us/height (iqr {r['us_per_height_iqr']:.1f}, kernel {r['kernel_ms']:.3f} ms, "
            f"{r['launches']} launches, {r['trials']} trials)")


def table(rows) -> None:
    print("\n| d | R | heights | window | pairs needed | fused us/height (iqr) / trials | host loop us/height (iqr) / trials |"
          " batch loop us/height (iqr) / trials | fused vs host loop | fused vs batch loop |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        f, h, b = r["fused"], r["host-loop"], r["batch-loop"]
        print(f"| {f['d']} | {f['rivals']} | {f['heights']} | 2^{f['window_log2']} | {f['pairs_needed']} | "
              f"{f['us_per_height']:.1f} ({f['us_per_height_iqr']:.1f}) / {f['trials']} | "
              f"{h['us_per_height']:.1f} ({h['us_per_height_iqr']:.1f}) / {h['trials']} | "
              f"{b['us_per_height']:.1f} ({b['us_per_height_iqr']:.1f}) / {b['trials']} | "
              f"{h['call_ms'] / f['call_ms']:.2f}x | {b['call_ms'] / f['call_ms']:.2f}x |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--heights", type=int, default=8)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.calls < 7:
        ap.error("--calls must be at least 7")
    rows, published, lanes_rows = [], [], []

    def three_ways(d, wlog, heights, rs, into):
        got = {w: measure(exes, w, d, wlog, heights, rs, a.calls) for w in WAYS}
        for R in rs:
            f = got["fused"][R]
            for w in WAYS:
                assert got[w][R]["checksum"] == f["checksum"], f"d={d} R={R}: fused and {w} mined different bytes"
            into.append({w: got[w][R] for w in WAYS})
            print(f"d={d} window=2^{wlog} R={R} heights={heights}: " + "  ".join(f"{w} {line(got[w][R])}" for w in WAYS),
                  flush=True)

    with tempfile.TemporaryDirectory() as td:
        exes = {lib: compile_bench(td, lib) for lib in ("pow_gpu", "pow_gpu_test")}
        for d in DS:
            three_ways(d, min(d + 7, 32), a.heights, RS, rows)
        three_ways(18, 32, 10, [3], published)
        for d in (13, 19):
            for lanes in (0, 2, 4):
                got = measure(exes, "fused", d, d + 7, a.heights, RS, a.calls, {"POW_RACE_LANES_LOG2": str(lanes)})
                for R, r in got.items():
                    lanes_rows.append({**r, "lanes_log2": lanes})
                    print(f"d={d} R={R} lanes_log2={lanes}: {line(r)}", flush=True)
    won = [d for d in DS if all(wins(r["fused"], r["host-loop"]) for r in rows if r["fused"]["d"] == d)]
    threshold = max(won) if won else -1
    losses = [d for d in DS if d < threshold and d not in won]
    table(rows)
    print("\nthe published shape:")
    table(published)
    print("\n| d | R | lanes_log2 | fused us/height (iqr) / trials |")
    print("|---|---|---|---|")
    for r in lanes_rows:
        print(f"| {r['d']} | {r['rivals']} | {r['lanes_log2']} | {r['us_per_height']:.1f} ({r['us_per_height_iqr']:.1f}) / "
              f"{r['trials']} |")
    print(f"\nfused beats the host loop beyond both interquartile ranges, at R = 3 and R = 64, at d in {won}; "
          f"POW_RACE_FUSED_MAX_D by the rule: {threshold}"
          + (f" (no win below it at d in {losses})" if losses else ""))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"rows": rows, "published": published, "lanes_rows": lanes_rows, "fused_wins_at": won,
                       "threshold_by_rule": threshold}, fh, indent=1)


if __name__ == "__main__":
    main()
