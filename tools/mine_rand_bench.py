#!/usr/bin/env python3
"""What replaying the reference's rand() nonces costs, on one GPU in one process:

  per call    pow_mine_rand (K8, the stream of srand(SEED) from trial 0) against
              pow_mine (counter nonces from 0) on the same N templates at d = 9,
              13, 17, 19, 21 and 23.  A sample is one pass over the N templates,
              divided by N; the two calls draw different nonces, so their trials
              to the answer differ template by template and agree only in the
              mean: the mean trials to the answer and the trials issued are
              printed beside the times.
  sustained   a 2^30-trial window at d = 32 that holds no solution (seeds are
              tried from --seed upwards until one qualifies), against pow_mine
              over a 2^30-counter window at d = 32 that holds none either.

Every value is the median of `--calls` (>= 7) samples after pow_warmup and one
discarded sample, with the interquartile range beside it.  Both calls go
through the same ctypes binding of the shipped library.

    python tools/mine_rand_bench.py [--calls 9] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mpi_blockchain_amd.block import make_block  # noqa: E402
from mpi_blockchain_amd.miner import GpuMiner  # noqa: E402

SEED = 1700000003
SIZES = [(9, 256), (13, 256), (17, 256), (19, 64), (21, 64), (23, 32)]


def quartiles(xs):
    q = statistics.quantiles(xs, n=4, method="inclusive")
    return statistics.median(xs), q[2] - q[0]


def templates(n: int, d: int):
    return [make_block(1 + i, i % 7, d, 1_700_000_000 + 17 * i, prev=(b"%064x" % (i * 0x9E3779B97F4A7C15 + d))) for i in range(n)]


def per_call(m: GpuMiner, d: int, n: int, calls: int) -> dict:
    tm = templates(n, d)
    out = {"d": d, "n": n}
    for way in ("rand", "counter"):
        samples, hashes, kernel_ms, to_answer = [], 0, 0.0, 0
        for k in range(calls + 1):
            hashes, kernel_ms, to_answer = 0, 0.0, 0
            t0 = time.perf_counter()
            for t in tm:
                r = m.mine_rand(t, SEED, 0, 1 << 32, d) if way == "rand" else m.mine(t, 0, 1 << 32, d)
                hashes += r.hashes
                kernel_ms += r.kernel_ms
                to_answer += (r.trial if way == "rand" else r.counter) + 1
            dt = time.perf_counter() - t0
            if k:
                samples.append(1e6 * dt / n)
        med, iqr = quartiles(samples)
        out[way] = {"us": med, "us_iqr": iqr, "kernel_us": 1e3 * kernel_ms / n, "trials_to_answer": to_answer / n,
                    "trials_issued": hashes / n, "samples_us": samples}
    out["ratio"] = out["rand"]["us"] / out["counter"]["us"]
    return out


def sustained(m: GpuMiner, seed0: int, calls: int) -> dict:
    tmpl = make_block(1, 0, 32, 1_700_000_000)
    n = 1 << 30
    seed = seed0
    while m.mine_rand(tmpl, seed, 0, n, 32) is not None:
        seed += 1
    start = 0
    while m.mine(tmpl, start, n, 32) is not None:
        start += n
    out = {"trials": n, "seed": seed, "counter_start": start}
    for way in ("rand", "counter"):
        samples, kernel, launches = [], [], 0
        for k in range(calls + 1):
            t0 = time.perf_counter()
            r = m.mine_rand(tmpl, seed, 0, n, 32) if way == "rand" else m.mine(tmpl, start, n, 32)
            dt = time.perf_counter() - t0
            assert r is None
            s = m.stats()
            assert s["hashes"] >= n, s  # every trial of the window was tested
            if k:
                samples.append(n / dt)
                kernel.append(n / (1e-3 * s["kernel_ms"]))
                launches = s["launches"]
        med, iqr = quartiles(samples)
        out[way] = {"trials_per_s": med, "trials_per_s_iqr": iqr, "kernel_trials_per_s": statistics.median(kernel),
                    "launches": launches, "samples": samples}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--seed", type=int, default=SEED)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.calls < 7:
        ap.error("--calls must be at least 7")
    with GpuMiner(0) as m:
        m.warmup()
        print("device:", m.device_info(), flush=True)
        rows = []
        for d, n in SIZES:
            r = per_call(m, d, n, a.calls)
            rows.append(r)
            print(f"d={d} n={n}: " + "  ".join(
                f"{w} {r[w]['us']:.1f} us/call (iqr {r[w]['us_iqr']:.1f}, kernel {r[w]['kernel_us']:.1f} us, "
                f"{r[w]['trials_to_answer']:.0f} trials to the answer, {r[w]['trials_issued']:.0f} issued)"
                for w in ("rand", "counter")) + f"  ratio {r['ratio']:.2f}", flush=True)
        sus = sustained(m, a.seed, a.calls)
    print("\n| d | n | pow_mine_rand us/call (iqr) | pow_mine us/call (iqr) | ratio | rand kernel us | counter kernel us |"
          " rand trials to answer / issued | counter trials to answer / issued |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        a_, c = r["rand"], r["counter"]
        print(f"| {r['d']} | {r['n']} | {a_['us']:.1f} ({a_['us_iqr']:.1f}) | {c['us']:.1f} ({c['us_iqr']:.1f}) | {r['ratio']:.2f} | "
              f"{a_['kernel_us']:.1f} | {c['kernel_us']:.1f} | {a_['trials_to_answer']:.0f} / {a_['trials_issued']:.0f} | "
              f"{c['trials_to_answer']:.0f} / {c['trials_issued']:.0f} |")
    print(f"\nsustained, 2^30 trials at d = 32 without a solution (seed {sus['seed']}; counters from {sus['counter_start']}):")
    for w in ("rand", "counter"):
        s = sus[w]
        print(f"  {w}: {s['trials_per_s'] / 1e9:.3f} G trials/s (iqr {s['trials_per_s_iqr'] / 1e9:.3f}), "
              f"kernel alone {s['kernel_trials_per_s'] / 1e9:.3f} G/s, {s['launches']} launches")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"seed": SEED, "rows": rows, "sustained": sus}, fh, indent=1)


if __name__ == "__main__":
    main()
