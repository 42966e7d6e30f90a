#!/usr/bin/env python3
"""Wall time per template of mining n independent templates, two ways, on one
GPU in one run:

  (a) fused   one pow_mine_batch call, K5 forced at every d (test library,
              POW_BATCH_FUSED_MAX=32)
  (b) c-loop  the loop around pow_mine, from C against the shipped library:
              what a caller had before pow_mine_batch (pow_mine is the same
              code before and after it)

Both mine the same templates (tools/mine_batch_bench.c), over the window 2^32
and over 2^(d + 7).  Every value is the median of `--calls` (>= 7) calls after
pow_warmup and one discarded call, with the interquartile range beside it; each
way runs in its own process.  The outputs of the two ways are compared: inside
the fused process byte for byte with pow_mine's (all 552 bytes and the counter
of every template), and across the processes by checksum.  A row of K5's
POW_BATCH_LANES_LOG2 {0, 2, 4} at d = 9 and 13 follows.

The rule for POW_BATCH_FUSED_MAX_D (csrc/pow_ctx.h) is applied to the result:
the largest measured d at which (a)'s median at n = 64 is below (b)'s by more
than the two interquartile ranges combined, with both windows; -1 if that does
not hold at the lowest d.

    python tools/mine_batch_bench.py [--calls 9] [--out FILE.json]

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
WAYS = {"fused": ("pow_gpu_test", "batch", {"POW_BATCH_FUSED_MAX": "32"}),
        "c-loop": ("pow_gpu", "loop", {})}


def sizes(d: int) -> list[int]:
    return [2, 8, 64, 1024 if d < 21 else 100]


def compile_bench(td: str, lib: str) -> str:
    exe = os.path.join(td, "mine_batch_bench_" + lib)
    subprocess.run(["gcc", "-std=c11", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "mine_batch_bench.c"), "-L", PKG, "-l" + lib, f"-Wl,-rpath,{PKG}",
                    "-o", exe], check=True)
    return exe


def quartiles(xs):
    q = statistics.quantiles(xs, n=4, method="inclusive")
    return statistics.median(xs), q[2] - q[0]


def measure(exes, way: str, d: int, wlog: int, ns, calls: int, extra_env=None) -> dict:
    """One process: every n of `ns` at (d, window).  {n: row}."""
    lib, mode, env = WAYS[way]
    p = subprocess.run(["timeout", "-k", "10", "300", exes[lib], mode, str(d), str(wlog), str(calls), *map(str, ns)],
                       capture_output=True, text=True, env={**os.environ, **env, **(extra_env or {})})
    if p.returncode != 0:
        sys.exit(f"{way} d={d} window=2^{wlog}: exit {p.returncode}\n{p.stdout}{p.stderr}")
    rows = {}
    for line in p.stdout.strip().splitlines():
        r = json.loads(line)
        assert r["equal"] != 0, f"{way} d={d} n={r['n']}: pow_mine_batch and pow_mine gave different bytes"
        med, iqr = quartiles(r["ms"])
        n = r["n"]
        rows[n] = {"way": way, "d": d, "window_log2": wlog, "n": n, "checksum": r["checksum"], "equal": r["equal"],
                   "call_ms": med, "call_ms_iqr": iqr, "us_per_template": 1e3 * med / n,
                   "us_per_template_iqr": 1e3 * iqr / n, "kernel_ms": statistics.median(r["kernel_ms"]),
                   "launches": int(statistics.median(r["launches"])), "samples_ms": r["ms"]}
    assert sorted(rows) == sorted(ns)
    return rows


def wins(f: dict, c: dict) -> bool:
    return c["call_ms"] - f["call_ms"] > c["call_ms_iqr"] + f["call_ms_iqr"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.calls < 7:
        ap.error("--calls must be at least 7")
    rows, lanes_rows = [], []
    with tempfile.TemporaryDirectory() as td:
        exes = {lib: compile_bench(td, lib) for lib in ("pow_gpu", "pow_gpu_test")}
        for d in DS:
            for wlog in (32, d + 7):
                got = {w: measure(exes, w, d, wlog, sizes(d), a.calls) for w in WAYS}
                for n in sizes(d):
                    f, c = got["fused"][n], got["c-loop"][n]
                    assert f["checksum"] == c["checksum"], f"d={d} n={n}: the two ways mined different bytes"
                    rows.append({"fused": f, "c-loop": c})
                    print(f"d={d} window=2^{wlog} n={n}: fused {f['us_per_template']:.2f} us/template "
                          f"(iqr {f['us_per_template_iqr']:.2f}, kernel {f['kernel_ms']:.3f} ms, {f['launches']} launches)  "
                          f"c-loop {c['us_per_template']:.2f} (iqr {c['us_per_template_iqr']:.2f}, "
                          f"kernel {c['kernel_ms']:.3f} ms, {c['launches']} launches)", flush=True)
        for d in (9, 13):
            for lanes in (0, 2, 4):
                got = measure(exes, "fused", d, d + 7, [64, 1024], a.calls, {"POW_BATCH_LANES_LOG2": str(lanes)})
                for n, r in got.items():
                    lanes_rows.append({**r, "lanes_log2": lanes})
                    print(f"d={d} window=2^{d + 7} n={n} lanes_log2={lanes}: {r['us_per_template']:.2f} us/template "
                          f"(iqr {r['us_per_template_iqr']:.2f})", flush=True)
    won = [d for d in DS if all(wins(r["fused"], r["c-loop"]) for r in rows
                                if r["fused"]["d"] == d and r["fused"]["n"] == 64)]
    threshold = max(won) if won and DS[0] in won else -1
    losses = [d for d in DS if d < threshold and d not in won]
    print("\n| d | window | n | fused us/template (iqr) | C loop us/template (iqr) | speed-up | fused kernel ms / launches |"
          " C loop kernel ms / launches |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        f, c = r["fused"], r["c-loop"]
        print(f"| {f['d']} | 2^{f['window_log2']} | {f['n']} | {f['us_per_template']:.2f} ({f['us_per_template_iqr']:.2f}) | "
              f"{c['us_per_template']:.2f} ({c['us_per_template_iqr']:.2f}) | {c['call_ms'] / f['call_ms']:.1f}x | "
              f"{f['kernel_ms']:.3f} / {f['launches']} | {c['kernel_ms']:.3f} / {c['launches']} |")
    print("\n| d | n | lanes_log2 | fused us/template (iqr) |")
    print("|---|---|---|---|")
    for r in lanes_rows:
        print(f"| {r['d']} | {r['n']} | {r['lanes_log2']} | {r['us_per_template']:.2f} ({r['us_per_template_iqr']:.2f}) |")
    print(f"\nfused beats the C loop at n = 64 beyond both interquartile ranges, with both windows, at d in {won}; "
          f"POW_BATCH_FUSED_MAX_D by the rule: {threshold}"
          + (f" (no win below it at d in {losses})" if losses else ""))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"rows": rows, "lanes_rows": lanes_rows, "fused_wins_at": won, "threshold_by_rule": threshold},
                      fh, indent=1)


if __name__ == "__main__":
    main()
