"""pow_find_seed (K9) where its first tests do not reach: the device's seeding
on a window of seeds through 2^31 with the two seeds whose Lehmer steps all
give zero, the digit edges of the two 62 x 62-bit prefilter tables, targets one
6-bit field away from a drawn nonce, and the most records one trial can make.
Every call goes through seed_util.check_against_ref (the brute force over
pow_rand_nonces, whole nonce by whole nonce); the targets and the expectations
stated beside it come from tests/rand_util.py, pure Python that shares no code
with the library.  tests/test_seed_host.py pins these inputs without a GPU."""
import pytest

import rand_util
import seed_util
from seed_util import call, check_against_ref, find_seed_ru, miner_with
from mpi_blockchain_amd import _lib
from mpi_blockchain_amd.miner import GpuMiner

pytestmark = pytest.mark.gpu

SEED = 1700000003


@pytest.fixture(scope="module")
def shipped():
    with GpuMiner(0) as m:
        yield m


# ---- a: the seeding ----
def test_seeds_through_2_pow_31(shipped):
    """64 seeds from 0x7FFFFFE0, one target each: the nonce of the seed at
    position p at trial 37 p mod 64.  Positions 31 to 33 are 0x7FFFFFFF,
    0x80000000 and 0x80000001."""
    first = 0x7FFFFFE0
    spots = [(p, 37 * p % 64) for p in range(64)]
    nonces = [seed_util.ru_stream(first + p, 0, 64)[t] for p, t in spots]
    want = [(first + p, p, t) for p, t in spots]
    assert [s for s, _, _ in want[31:34]] == [0x7FFFFFFF, 0x80000000, 0x80000001]
    assert find_seed_ru(nonces, first, 64, 0, 64) == want
    assert check_against_ref(shipped, nonces, first, 64, 0, 64) == want


@pytest.mark.parametrize("seed", seed_util.DEGENERATE)
def test_degenerate_seeds_at_a_deep_start(shipped, seed):
    """r[1..30] all zero, and the launch's jump polynomial applied to that state."""
    start = seed_util.DEEP
    stream = seed_util.ru_stream(seed, start, 64)
    trials = [0, 30, 31, 32, 63]
    want = [(seed, k, start + t) for k, t in enumerate(trials)]
    nonces = [stream[t] for t in trials]
    assert find_seed_ru(nonces, seed, 1, start, 64) == want
    assert check_against_ref(shipped, nonces, seed, 1, start, 64) == want
    assert check_against_ref(shipped, list(stream), seed, 1, start, 64) == [(seed, t, start + t) for t in range(64)]


# ---- b: the digit edges of the prefilter ----
def test_prefilter_digit_edges(shipped):
    """Targets chosen by their digits: 0 and 61 (bits 0 and 61 of a table's
    word) and 31 | 32 (the seam of its halves), in the first pair (`pair`) and
    in the second (`pair2`)."""
    hits = seed_util.digit_edge_hits()
    assert len(hits) == 12 and all(hits.values()), hits
    nonces = [n for _, _, n in hits.values()]
    want = find_seed_ru(nonces, seed_util.EDGE_SEEDS[0], 3, 0, seed_util.EDGE_TRIALS)
    assert sorted(want) == sorted((s, k, t) for k, (s, t, _) in enumerate(hits.values()))
    assert check_against_ref(shipped, nonces, seed_util.EDGE_SEEDS[0], 3, 0, seed_util.EDGE_TRIALS) == want


# ---- c: near misses ----
@pytest.mark.parametrize("switches", [{}, {"POW_SEED_RUN": 31, "POW_SEED_WG": 2}], ids=["shipped", "run31_wg2"])
def test_near_misses(shipped, switches):
    """Eleven targets that a trial's digits pass a table with, or all but one
    6-bit field of, and the nonce itself: one match."""
    stream = seed_util.ru_stream(SEED, 0, 2048)
    n = stream[1007]
    assert n == b"99Z0FmjmU"
    nonces = seed_util.near_misses(n, stream[5], stream[6])
    want = [(SEED, 11, 1007)]
    assert find_seed_ru(nonces, SEED, 1, 0, 2048) == want
    if not switches:
        assert check_against_ref(shipped, nonces, SEED, 1, 0, 2048) == want
    else:
        with miner_with(**switches) as m:
            assert check_against_ref(m, nonces, SEED, 1, 0, 2048) == want


# ---- d: many records of one trial ----
def test_64_equal_targets_under_seeds_0_and_1(shipped):
    """128 records of two lanes' one trial, in the order the host promises:
    the seed's position, the trial, the target."""
    nonces = [rand_util.nonces(1, 5, 1)[0]] * 64
    want = [(s, k, 5) for s in (0, 1) for k in range(64)]
    assert find_seed_ru(nonces, 0xFFFFFFFE, 4, 0, 64) == want
    assert check_against_ref(shipped, nonces, 0xFFFFFFFE, 4, 0, 64, cap=256) == want
    rc, got, n_found, pairs, untouched = call(shipped, nonces, 0xFFFFFFFE, 4, 0, 64, cap=100)
    assert (rc, got, n_found, pairs, untouched) == (_lib.POW_ENOSPC, want[:100], 128, 4 * 64, True)
