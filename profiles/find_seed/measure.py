"""Measure pow_find_seed (K9) on the GPU against the reference's own loop on the CPU.

    python profiles/find_seed/measure.py [--out FILE.json] [--quick]

1. The call at n_seeds in {1, 64, 4096} x trial_count in {2^20, 2^26, 2^32}, one
   target and 64 targets: medians of 9 calls (calls longer than 5 s: of 3; longer
   than 20 s: one), wall and kernel ms.  At 4,096 seeds the count goes up by
   factors of four from 2^26 while the next step is expected within a minute.
   Every call holds one target that is in the window, at its last pair, and the
   call must find exactly that.
2. The launch cap: one launch of 2^L pairs, L = 30 down to 26, through the test
   library's POW_SEED_LAUNCH_LOG2, in two shapes (16 seeds x 2^26 trials; 1,024
   seeds x 2^20), beside K8's full launch (pow_mine_rand over 2^26 trials at d =
   32) in the same process.
3. The baseline: the same search by the reference's own srand + gen_random_nonce
   (oracle/_ref/libref_O2.so, which build() makes where the reference's source
   is), driven by a small C loop compiled here so that no interpreter stands
   between two draws.  One core; seeds x trials sized to about a second.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from mpi_blockchain_amd import _lib  # noqa: E402
from mpi_blockchain_amd.block import make_block  # noqa: E402
from mpi_blockchain_amd.miner import GpuMiner, rand_nonces  # noqa: E402

SEED = 1700000003

DRIVER = r"""
#include <dlfcn.h>
#include <stdint.h>
#include <string.h>
/* seeds [first, first + n_seeds), `count` trials each, against n_targets nonces of 10 bytes: matches */
uint64_t ref_search(const char* lib, uint32_t first, uint32_t n_seeds, uint64_t count, const char* targets, int n_targets) {
  void* h = dlopen(lib, RTLD_NOW | RTLD_LOCAL);
  if (!h) return ~0ull;
  void (*seed)(unsigned) = (void (*)(unsigned))dlsym(h, "ref_srand");
  void (*draw)(char*) = (void (*)(char*))dlsym(h, "ref_gen_random_nonce");
  if (!seed || !draw) return ~0ull;
  uint64_t found = 0;
  char nonce[16];
  for (uint32_t p = 0; p < n_seeds; ++p) {
    seed(first + p);
    for (uint64_t t = 0; t < count; ++t) {
      draw(nonce);
      for (int k = 0; k < n_targets; ++k) found += memcmp(nonce, targets + 10 * k, 9) == 0;
    }
  }
  return found;
}
"""


def targets_for(seed_first, n_seeds, count, n_targets):
    """One nonce of the window, at its last pair, then nonces of a seed far outside it."""
    hit = rand_nonces(seed_first + n_seeds - 1, count - 1, 1)
    return hit + rand_nonces(seed_first ^ 0x40000000, 0, n_targets - 1)


def one_call(m, nonces, seed_first, n_seeds, count):
    t0 = time.perf_counter()
    got = m.find_seed(nonces, seed_first, n_seeds, 0, count)
    wall = (time.perf_counter() - t0) * 1e3
    assert [(g.seed, g.trial, g.target) for g in got] == [(seed_first + n_seeds - 1, count - 1, 0)], got
    s = m.stats()
    assert s["hashes"] == n_seeds * count
    return wall, s["kernel_ms"], s["launches"]


def measure(m, seed_first, n_seeds, count, n_targets, reps=9):
    nonces = targets_for(seed_first, n_seeds, count, n_targets)
    first = one_call(m, nonces, seed_first, n_seeds, count)  # also the warm-up where it is short
    reps = 1 if first[0] > 20e3 else 3 if first[0] > 5e3 else reps
    runs = [first] if reps == 1 else [one_call(m, nonces, seed_first, n_seeds, count) for _ in range(reps)]
    wall, kern = statistics.median(r[0] for r in runs), statistics.median(r[1] for r in runs)
    row = {"n_seeds": n_seeds, "log2_count": count.bit_length() - 1, "targets": n_targets, "calls": reps,
           "wall_ms": wall, "kernel_ms": kern, "launches": runs[0][2], "gpairs_per_s": n_seeds * count / kern / 1e6}
    print(json.dumps(row), flush=True)
    return row


def launch_cap(rows):
    tmpl = make_block(1, 0, 32, 1700000000)
    os.environ.pop("POW_SEED_LAUNCH_LOG2", None)
    for log2 in (30, 29, 28, 27, 26):
        os.environ["POW_SEED_LAUNCH_LOG2"] = str(log2)
        with GpuMiner(0, test_hooks=True) as m:
            k8, seed = [], SEED
            while m.mine_rand(tmpl, seed, 0, 1 << 26, 32) is not None:  # a full launch: one without a solution
                seed += 1
            for _ in range(10):
                assert m.mine_rand(tmpl, seed, 0, 1 << 26, 32) is None
                s = m.stats()
                assert s["launches"] == 1
                k8.append(s["kernel_ms"])
            for n_seeds, count in ((16, 1 << 26), (1024, 1 << 20)):
                nonces = targets_for(SEED, n_seeds, count, 64)
                runs = [one_call(m, nonces, SEED, n_seeds, count) for _ in range(10)][1:]
                per = statistics.median(r[1] / r[2] for r in runs)
                row = {"launch_log2": log2, "n_seeds": n_seeds, "log2_count": count.bit_length() - 1, "launches": runs[0][2],
                       "k9_ms_per_launch": per, "k8_full_launch_ms": statistics.median(k8[1:])}
                print(json.dumps(row), flush=True)
                rows.append(row)
    os.environ.pop("POW_SEED_LAUNCH_LOG2", None)


def baseline(rows):
    ref = os.path.join(ROOT, "oracle", "_ref", "libref_O2.so")
    if not os.path.exists(ref):
        print("no oracle/_ref/libref_O2.so: the baseline is not measured", flush=True)
        return
    with tempfile.TemporaryDirectory() as td:
        src, so = os.path.join(td, "ref_search.c"), os.path.join(td, "ref_search.so")
        open(src, "w").write(DRIVER)
        subprocess.run(["gcc", "-O2", "-shared", "-fPIC", src, "-ldl", "-o", so], check=True)
        D = ctypes.CDLL(so)
        D.ref_search.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_char_p,
                                 ctypes.c_int]
        D.ref_search.restype = ctypes.c_uint64
        for n_seeds, count in ((1, 1 << 22), (64, 1 << 16)):
            for n_targets in (1, 64):
                buf = b"".join(targets_for(SEED, n_seeds, count, n_targets))
                times = []
                for _ in range(5):
                    t0 = time.perf_counter()
                    found = D.ref_search(ref.encode(), SEED, n_seeds, count, buf, n_targets)
                    times.append((time.perf_counter() - t0) * 1e3)
                    assert found == 1, found
                ms = statistics.median(times)
                row = {"reference_cpu": True, "n_seeds": n_seeds, "log2_count": count.bit_length() - 1, "targets": n_targets,
                       "calls": 5, "wall_ms": ms, "mpairs_per_s": n_seeds * count / ms / 1e3}
                print(json.dumps(row), flush=True)
                rows.append(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also keep the rows in this JSON file")
    ap.add_argument("--quick", action="store_true", help="no call above 2^32 pairs")
    a = ap.parse_args()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = {"table": [], "launch_cap": [], "baseline": []}

    def save():
        if a.out:
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)

    baseline(out["baseline"])
    save()
    launch_cap(out["launch_cap"])
    save()
    with GpuMiner(0) as m:
        info = m.device_info()
        out["device"] = info
        print(json.dumps(info), flush=True)
        for n_targets in (1, 64):
            for n_seeds in (1, 64):
                for log2 in (20, 26, 32):
                    out["table"].append(measure(m, SEED, n_seeds, 1 << log2, n_targets))
                    save()
            out["table"].append(measure(m, SEED, 4096, 1 << 20, n_targets))
            save()
            log2 = 26
            while log2 <= 32 and not (a.quick and log2 > 20):
                row = measure(m, SEED, 4096, 1 << log2, n_targets)
                out["table"].append(row)
                save()
                if row["wall_ms"] * 4 > 60e3:  # the next step would not finish within a minute
                    break
                log2 += 2
    save()


if __name__ == "__main__":
    main()
