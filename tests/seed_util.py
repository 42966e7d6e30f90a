"""What the tests of pow_find_seed (K9) share: the brute force built on
pow_rand_nonces (pinned to the reference's own gen_random_nonce by
tests/golden/rand_replay.json: tests/test_rand_host.py and test_seed_host.py),
contexts of the test library under its three switches and the call through the C
ABI with a poisoned output."""
import ctypes
import functools
import json
import os

import helpers
from mpi_blockchain_amd import _lib
from mpi_blockchain_amd.miner import rand_nonces

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("POW_SEED_RUN", "POW_SEED_WG", "POW_SEED_LAUNCH_LOG2")
LIMIT = 1 << 56
POISON = 0xA5


@functools.lru_cache(maxsize=None)
def replay():
    with open(os.path.join(ROOT, "tests", "golden", "rand_replay.json")) as f:
        return json.load(f)


def golden_nonces(seed: int) -> list[bytes]:
    """The reference's first 64 nonces after srand(seed), as recorded."""
    return [bytes.fromhex(h) for h in replay()["nonces"][str(seed)]]


@functools.lru_cache(maxsize=None)
def stream(seed: int, start: int, count: int) -> tuple:
    """pow_rand_nonces, nine characters per trial; computed once per window."""
    return tuple(n[:9] for n in rand_nonces(seed, start, count))


def nonce_at(seed: int, trial: int) -> bytes:
    return rand_nonces(seed, trial, 1)[0]


def find_seed_ref(nonces, seed_first: int, n_seeds: int, start: int, count: int) -> list[tuple]:
    """Every (seed, target, trial) of the request by brute force, in the call's
    order: by position of the seed in the window, then trial, then target."""
    want: dict = {}
    for k, n in enumerate(nonces):
        want.setdefault(bytes(n)[:9], []).append(k)
    out = []
    for p in range(n_seeds):
        seed = (seed_first + p) & 0xFFFFFFFF
        for t, n in enumerate(stream(seed, start, count)):
            for k in want.get(n, ()):
                out.append((seed, k, start + t))
    return out


def miner_with(**switches):
    """A context of the test library whose pow_init saw the given switches."""
    return helpers.hooked_miner(SWITCHES, **switches)


def pack(nonces) -> bytes:
    return b"".join(bytes(n)[:9].ljust(9, b"\0") + b"\0" for n in nonces)


def call(m, nonces, seed_first, n_seeds, start, count, cap=256, cancel=None, epoch=0, ctx="own"):
    """pow_find_seed through the C ABI with a poisoned output: rc, the matches
    as (seed, target, trial) up to min(n_found, cap), n_found, pairs and the
    untouched tail of `out` as a bool."""
    L = m.L if m is not None else _lib.load()
    out = (_lib.SeedMatchRec * max(cap, 1))()
    ctypes.memset(out, POISON, ctypes.sizeof(out))
    n_found, pairs = ctypes.c_size_t(12345), ctypes.c_uint64(12345)
    rc = L.pow_find_seed(m.ctx if ctx == "own" else ctx, pack(nonces), len(nonces), seed_first & 0xFFFFFFFF, n_seeds,
                         start, count, cancel, epoch, out, cap, ctypes.byref(n_found), ctypes.byref(pairs))
    n = min(n_found.value, cap) if rc in (1, _lib.POW_ENOSPC) else 0
    got = [(out[i].seed, out[i].target, out[i].trial) for i in range(n)]
    tail = bytes(out)[n * ctypes.sizeof(_lib.SeedMatchRec):]
    return rc, got, n_found.value, pairs.value, tail == bytes([POISON]) * len(tail)


def check_against_ref(m, nonces, seed_first, n_seeds, start, count, cap=256):
    """One call against the brute force: the same matches in the same order.  Returns them."""
    want = find_seed_ref(nonces, seed_first, n_seeds, start, count)
    rc, got, n_found, pairs, tail_ok = call(m, nonces, seed_first, n_seeds, start, count, cap)
    assert rc == (1 if want else 0), (rc, m.L.pow_last_error(), seed_first, n_seeds, start, count)
    assert (got, n_found) == (want, len(want)), (got, want)
    assert pairs == n_seeds * count and tail_ok
    return got
