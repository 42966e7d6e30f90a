"""Generate tests/golden/rand_seam.json: trials of the reference's nonce stream
whose digests sit on the two sides of the 32-bit difficulty seam, where
pow_mine_rand (K8) compares H0 <= thr with thr = 1 (d = 31) and thr = 0
(d = 32).  The rows of lz_witnesses.json are counters and do not apply: K8's
nonces are rand()'s.

    python tests/golden/gen_rand_seam.py   # needs the GPU

For template S0 of golden.json and the seed of the GPU tests, pow_mine_rand
searches at d = 31 from trial 0, each call from behind the last hit, until it
has one trial with exactly 31 leading zero bits (H0 = 1) and one with at least
32 (H0 = 0).  The search is only a search: every nonce written is
tests/rand_util.py's, every digest hashlib's, and the tests check every row
with both again before they use it.  Each witness's 2,048-trial window
[trial - 1000, trial - 1000 + 2048) holds no other trial with 29 or more zero
bits (rand_util and hashlib, 2,048 hashes per witness).
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import rand_util  # noqa: E402
from helpers import block_from_template  # noqa: E402

OUT = os.path.join(HERE, "rand_seam.json")
TEMPLATE, SEED = "S0", 1700000003
BEFORE, WINDOW = 1000, 2048
MAX_CALLS = 64  # 2^31 trials per hit expected, every other hit on either side of the seam


def lz_of(digest: bytes) -> int:
    return 256 - int.from_bytes(digest, "big").bit_length()


def row(tb: bytes, trial: int) -> dict:
    nonce, = rand_util.nonces(SEED, trial, 1)
    dg = hashlib.sha256(rand_util.message(tb, nonce)).digest()
    return {"seed": SEED, "template": TEMPLATE, "trial": trial, "nonce": nonce[:9].decode(), "digest": dg.hex(),
            "leading_zeros": lz_of(dg)}


def lonely(tb: bytes, trial: int) -> bool:
    """No other trial of the witness's window has 29 or more leading zero bits."""
    hits = rand_util.mine(tb, SEED, trial - BEFORE, WINDOW, 29, want=WINDOW)
    return [h[0] for h in hits] == [trial]


def main():
    import ctypes

    from mpi_blockchain_amd.miner import GpuMiner

    with open(os.path.join(HERE, "golden.json")) as f:
        tmpl = block_from_template({t["name"]: t for t in json.load(f)["templates"]}[TEMPLATE])
    tb = ctypes.string_at(ctypes.addressof(tmpl), ctypes.sizeof(tmpl))
    exactly31 = at_least32 = None
    at, calls = 0, 0
    with GpuMiner(0) as m:
        while exactly31 is None or at_least32 is None:
            if calls == MAX_CALLS:
                raise SystemExit(f"no pair of witnesses in {MAX_CALLS} calls, up to trial {at}: "
                                 f"31 -> {exactly31}, 32+ -> {at_least32}")
            calls += 1
            hit = m.mine_rand(tmpl, SEED, at, 1 << 32, 31)
            if hit is None:
                at += 1 << 32
                continue
            at = hit.trial + 1
            r = row(tb, hit.trial)
            assert r["leading_zeros"] >= 31, r  # hashlib agrees that it is a hit at all
            if hit.trial < BEFORE or not lonely(tb, hit.trial):
                continue
            if r["leading_zeros"] == 31 and exactly31 is None:
                exactly31 = r
            if r["leading_zeros"] >= 32 and at_least32 is None:
                at_least32 = r
    out = {"before": BEFORE, "window": WINDOW, "calls": calls, "searched_to": at, "witnesses": [exactly31, at_least32]}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
