#!/usr/bin/env python3
"""Wall time per block of mining a chain, three ways, on one GPU in one run:

  (a) fused   one pow_mine_chain call, K4 forced at every d (test library,
              POW_CHAIN_FUSED_MAX=32)
  (b) host    the same call with the library's host loop forced (test library,
              POW_CHAIN_FUSED_MAX=-1)
  (c) c-loop  the loop of examples/mine_chain.c around pow_mine, from C against
              the shipped library: what a caller had before pow_mine_chain

All three mine the same chain (tools/mine_chain_bench.c).  Every value is the
median of `--calls` (>= 7) calls after pow_warmup and one discarded call, with
the interquartile range beside it.  The rule for POW_CHAIN_FUSED_MAX_D
(csrc/pow_ctx.h) is applied to the result: the largest measured d at which (a)'s
median is below (b)'s by more than the two interquartile ranges combined.

    python tools/mine_chain_bench.py [--calls 9] [--out FILE.json]

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
SIZES = [(9, 1000), (13, 1000), (17, 1000), (19, 100), (21, 100), (23, 100)]
WAYS = {"fused": ("pow_gpu_test", "chain", {"POW_CHAIN_FUSED_MAX": "32"}),
        "host": ("pow_gpu_test", "chain", {"POW_CHAIN_FUSED_MAX": "-1"}),
        "c-loop": ("pow_gpu", "loop", {})}


def compile_bench(td: str, lib: str) -> str:
    exe = os.path.join(td, "mine_chain_bench_" + lib)
    subprocess.run(["gcc", "-std=c11", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "mine_chain_bench.c"), "-L", PKG, "-l" + lib, f"-Wl,-rpath,{PKG}",
                    "-o", exe], check=True)
    return exe


def quartiles(xs):
    q = statistics.quantiles(xs, n=4, method="inclusive")
    return statistics.median(xs), q[2] - q[0]


def measure(exes, way: str, d: int, n: int, calls: int) -> dict:
    lib, mode, env = WAYS[way]
    p = subprocess.run(["timeout", "-k", "10", "240", exes[lib], mode, str(d), str(n), str(calls)],
                       capture_output=True, text=True, env={**os.environ, **env})
    if p.returncode != 0:
        sys.exit(f"{way} d={d} n={n}: exit {p.returncode}\n{p.stdout}{p.stderr}")
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r["valid"] == 1, r
    med, iqr = quartiles(r["ms"])
    return {"way": way, "d": d, "n": n, "tip": r["tip"], "call_ms": med, "call_ms_iqr": iqr,
            "us_per_block": 1e3 * med / n, "us_per_block_iqr": 1e3 * iqr / n,
            "kernel_ms": statistics.median(r["kernel_ms"]), "launches": int(statistics.median(r["launches"])),
            "samples_ms": r["ms"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.calls < 7:
        ap.error("--calls must be at least 7")
    rows = []
    with tempfile.TemporaryDirectory() as td:
        exes = {lib: compile_bench(td, lib) for lib in ("pow_gpu", "pow_gpu_test")}
        for d, n in SIZES:
            got = {w: measure(exes, w, d, n, a.calls) for w in WAYS}
            assert len({g["tip"] for g in got.values()}) == 1, "the three ways mined different chains"
            rows.append(got)
            print(f"d={d} n={n}: " + "  ".join(f"{w} {g['us_per_block']:.1f} us/block (iqr {g['us_per_block_iqr']:.1f}, "
                                                 f"kernel {g['kernel_ms']:.2f} ms, {g['launches']} launches)"
                                                 for w, g in got.items()), flush=True)
        published = measure(exes, "fused", 18, 10, a.calls)
    wins = [r["fused"]["d"] for r in rows
            if r["host"]["call_ms"] - r["fused"]["call_ms"] > r["host"]["call_ms_iqr"] + r["fused"]["call_ms_iqr"]]
    first = rows[0]
    beats_c_loop = first["c-loop"]["call_ms"] - first["fused"]["call_ms"] > \
        first["c-loop"]["call_ms_iqr"] + first["fused"]["call_ms_iqr"]
    threshold = max(wins) if wins and beats_c_loop else -1
    losses = [r["fused"]["d"] for r in rows if r["fused"]["d"] < threshold and r["fused"]["d"] not in wins]
    print("\n| d | n | fused us/block (iqr) | host loop us/block (iqr) | C loop us/block (iqr) | fused kernel ms / launches |"
          " host kernel ms / launches | C loop kernel ms / launches |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        f, h, c = r["fused"], r["host"], r["c-loop"]
        print(f"| {f['d']} | {f['n']} | {f['us_per_block']:.1f} ({f['us_per_block_iqr']:.1f}) | "
              f"{h['us_per_block']:.1f} ({h['us_per_block_iqr']:.1f}) | {c['us_per_block']:.1f} ({c['us_per_block_iqr']:.1f}) | "
              f"{f['kernel_ms']:.2f} / {f['launches']} | {h['kernel_ms']:.2f} / {h['launches']} | "
              f"{c['kernel_ms']:.2f} / {c['launches']} |")
    print(f"\n10 blocks at d = 18, one fused call: {published['call_ms']:.3f} ms (iqr {published['call_ms_iqr']:.3f}), "
          f"kernel {published['kernel_ms']:.3f} ms")
    print(f"fused beats the host loop beyond both interquartile ranges at d in {wins}; "
          f"beats the C loop at d = {first['fused']['d']}: {beats_c_loop}; POW_CHAIN_FUSED_MAX_D by the rule: {threshold}"
          + (f" (no win below it at d in {losses})" if losses else ""))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"rows": rows, "published_10_blocks_d18": published, "fused_wins_at": wins,
                       "beats_c_loop_at_first_d": beats_c_loop, "threshold_by_rule": threshold}, fh, indent=1)


if __name__ == "__main__":
    main()
