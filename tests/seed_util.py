"""What the tests of pow_find_seed (K9) share: the brute force built on
pow_rand_nonces (pinned to the reference's own gen_random_nonce by
tests/golden/rand_replay.json: tests/test_rand_host.py and test_seed_host.py),
the same search over tests/rand_util.py's pure-Python stream, the inputs the
edge tests share (chosen by their digits, from rand_util alone), contexts of the
test library under its three switches and the call through the C ABI with a
poisoned output."""
import ctypes
import functools
import json
import os

import helpers
import rand_util
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


@functools.lru_cache(maxsize=None)
def ru_stream(seed: int, start: int, count: int) -> tuple:
    """tests/rand_util.py's nonces of a window, nine characters per trial: pure
    Python, no code of the library's."""
    return tuple(n[:9] for n in rand_util.nonces(seed, start, count))


def find_seed_ru(nonces, seed_first: int, n_seeds: int, start: int, count: int) -> list[tuple]:
    """find_seed_ref's result from rand_util's stream instead of pow_rand_nonces'."""
    out = []
    for p in range(n_seeds):
        seed = (seed_first + p) & 0xFFFFFFFF
        for t, n in enumerate(ru_stream(seed, start, count)):
            out += [(seed, k, start + t) for k, target in enumerate(nonces) if bytes(target)[:9] == n]
    return out


def digits(nonce: bytes) -> list[int]:
    """A nonce's nine characters as positions in the alphabet: K9's 6-bit fields."""
    return [rand_util.ALPHABET.index(c) for c in bytes(nonce)[:9]]


def first_with_digits(at: int, pair, seeds, count: int):
    """(seed, trial, nonce) of the first trial of [0, count), seed by seed,
    whose digits at `at` and `at + 1` are `pair`; None if there is none."""
    for seed in seeds:
        for t, n in enumerate(ru_stream(seed, 0, count)):
            if (rand_util.ALPHABET.index(n[at]), rand_util.ALPHABET.index(n[at + 1])) == tuple(pair):
                return seed, t, n
    return None


# ---- the inputs tests/test_seed_edges_gpu.py and tests/test_seed_host.py share, all from rand_util ----
DEGENERATE = (0x7FFFFFFF, 0x80000001)  # Schrage's first step gives 0: r[1..30] are all zero
DEEP = (1 << 40) + 7
EDGE_SEEDS, EDGE_TRIALS = (1700000003, 1700000004, 1700000005), 4096
# digit 61 is bit 61 of a table's 64-bit word; 31 | 32 is the seam of its 32-bit halves
EDGE_PAIRS = ((0, 0), (61, 61), (0, 61), (61, 0), (31, 32), (32, 31))


def digit_edge_hits() -> dict:
    """(digit position, pair) -> (seed, trial, nonce) or None: the first trial
    of the edge window whose first two digits (the table `pair`) or third and
    fourth (`pair2`) are an edge pair."""
    return {(at, pair): first_with_digits(at, pair, EDGE_SEEDS, EDGE_TRIALS) for at in (0, 2) for pair in EDGE_PAIRS}


def near_misses(n: bytes, a: bytes, b: bytes) -> list[bytes]:
    """Twelve targets around the nonce n, with a and b two other nonces: n's
    first pair on a's tail (passes `pair` only); b's first pair, n's second and
    b's tail (with the first, a trial of n passes both tables through two
    targets and equals neither); n with each one of its nine characters
    replaced by the alphabet's next; n itself, last."""
    A = rand_util.ALPHABET
    out = [n[:2] + a[2:9], b[:2] + n[2:4] + b[4:9]]
    out += [n[:k] + bytes([A[(A.index(n[k]) + 1) % 62]]) + n[k + 1:9] for k in range(9)]
    return out + [n[:9]]


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
