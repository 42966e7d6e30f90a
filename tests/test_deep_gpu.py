"""K4, K5 and K6 (pow_mine_chain, pow_mine_batch, pow_mine_race) at deep
relative counters.  Their own suites hash every counter below the answer with
hashlib and so stay below rel = 2^18; the stretch of
tests/golden/deep_stretch.json is certified empty by the CPU oracle over at
least 62^5 + 2^20 counters before its solution b at d = 30, so a kernel started
inside it must walk to b.  The rows (deep_util.rows):

  far         from the stretch's first counter: every digit of rel, about 10^9 trials
  max_window  the same start, ctr_count = 2^32 exactly (zero in 32 bits)
  one         rel = 62^5: digits 1,0,0,0,0,0
  nines       rel = 62^5 - 1: five digits of 61, every carry
  step3, 4    rel = 62^3 and 62^4: single digits
  key_over    rel = 2^24: K6's key rel << 8 | rival needs 33 bits ...
  key_under   ... and rel = 2^24 - 1: 32
  edge_last   rel = 2^24 with the solution as the window's last counter
  edge_none   the same window one counter shorter: nothing to find

Every expected byte is hashlib's (deep_util, test_deep_host.py).  The fused
kernels are forced with POW_{CHAIN,BATCH,RACE}_FUSED_MAX=32 on the test
library unless a test says otherwise."""
import pytest

from mpi_blockchain_amd.miner import GpuMiner

import batch_util as bu
import chain_util as cu
import deep_util as du
import race_util as ru

pytestmark = pytest.mark.gpu

FILL = b"\xA5" * cu.BLOCK_BYTES


@pytest.fixture(scope="module")
def fused():
    with du.miner_with(**du.FUSED) as m:
        yield m


def chain_row(m, row, launches=None):
    """pow_mine_chain, one block, over a row; returns what the paths must agree in."""
    s = du.stretch()
    start, count, solves = du.rows()[row]
    rc, mined, hashes, out = cu.call(m.L, m.ctx, du.parent(), 1, s["difficulty"], s["owner"], [s["created_at"]], start, count)
    st = m.stats()
    assert st["hashes"] == hashes
    if launches is not None:
        assert st["launches"] == launches
        assert hashes <= count  # a lane tests a counter at most once
    if not solves:
        assert (rc, mined) == (0, 0), (rc, mined, m.L.pow_last_error())
        assert cu.raw(out) == FILL and hashes >= count
        return None
    assert (rc, mined) == (1, 1), (rc, mined, m.L.pow_last_error())
    assert cu.raw(out) == du.stated_chain()  # all 552 bytes; the nonce in them is found_ctr == b
    assert hashes >= s["counter"] - start + 1
    return cu.raw(out)


def batch_row(m, row, launches=None):
    """pow_mine_batch with the templates of owners 5 and 261 over a row."""
    s = du.stretch()
    start, count, solves = du.rows()[row]
    rc, solved, hashes, ctrs, out = bu.call(m.L, m.ctx, [du.template(o) for o in du.OWNERS], s["difficulty"], start, count)
    st = m.stats()
    assert st["hashes"] == hashes
    if launches is not None:
        assert st["launches"] == launches
        assert hashes <= 2 * count
    if not solves:
        assert (rc, solved) == (0, 0), (rc, solved, m.L.pow_last_error())
        assert ctrs == [bu.NONE] * 2 and bytes(out) == FILL * 2 and hashes >= 2 * count
        return None
    want_bytes, want_ctrs = du.stated_batch()
    assert (rc, solved) == (1, 2), (rc, solved, m.L.pow_last_error())
    assert ctrs == want_ctrs == [s["counter"]] * 2
    assert bytes(out) == want_bytes
    assert hashes >= 2 * (s["counter"] - start + 1)
    return bytes(out), ctrs


def race_row(m, row, owners=(5, 261), launches=None):
    """pow_mine_race, one height, rivals with equal created_at, over a row."""
    s = du.stretch()
    start, count, solves = du.rows()[row]
    R = len(owners)
    rc, mined, hashes, winners, ctrs, out = ru.call(m.L, m.ctx, du.parent(), 1, s["difficulty"], list(owners),
                                                    [s["created_at"]] * R, start, count)
    st = m.stats()
    assert st["hashes"] == hashes
    if launches is not None:
        assert st["launches"] == launches
        assert hashes <= R * count
    if not solves:
        assert (rc, mined) == (0, 0), (rc, mined, m.L.pow_last_error())
        assert winners == [ru.UNSET_WINNER] and ctrs == [ru.UNSET_CTR] and bytes(out) == FILL
        assert hashes >= R * count
        return None
    want_bytes, want_winners, want_ctrs = du.stated_race(tuple(owners))
    assert (rc, mined) == (1, 1), (rc, mined, m.L.pow_last_error())
    assert winners == want_winners == [0] and ctrs == want_ctrs == [s["counter"]]  # the tie goes to position 0
    assert bytes(out) == want_bytes and out[0].node_owner_number == owners[0]
    # every pair below the answer was tested, and the answer itself (position 0)
    assert hashes >= (s["counter"] - start) * R + 1
    return bytes(out), winners, ctrs


# ---- the rows, kernel by kernel ----
@pytest.mark.parametrize("row", du.ROW_NAMES)
def test_chain_at_depth(fused, row):
    chain_row(fused, row, launches=1)


@pytest.mark.parametrize("row", du.ROW_NAMES)
def test_batch_at_depth(fused, row):
    # a tile holds about 2^26 trials, expected (2^30 per template at d = 30) or the window's if
    # fewer: both templates in one launch where the window is 2^25 counters at most, else one each
    batch_row(fused, row, launches=1 if du.rows()[row][1] <= 1 << 25 else 2)


@pytest.mark.parametrize("row", du.ROW_NAMES)
def test_race_at_depth(fused, row):
    race_row(fused, row, launches=1)


@pytest.mark.parametrize("row", du.SWAPPED_ROWS)
def test_race_at_depth_with_the_rivals_swapped(fused, row):
    race_row(fused, row, owners=(261, 5), launches=1)


def test_one_rival_is_the_chain_at_depth(fused):
    """n_rivals = 1 goes through pow_mine_chain; found_ctr comes back out of the nonce."""
    race_row(fused, "step4", owners=(5,), launches=1)


# ---- the paths agree at depth ----
@pytest.mark.parametrize("call", ["chain", "batch", "race"])
def test_paths_agree_at_depth(call):
    """The far row on the shipped library (fused above d = 23 nowhere: the host
    loops over pow_mine) and on the test library with the fused paths switched
    off: the bytes and counters of the statements, as the fused kernels'."""
    run = {"chain": chain_row, "batch": batch_row, "race": race_row}[call]
    with GpuMiner(0) as m:
        shipped = run(m, "far")
    with du.miner_with(**du.LOOPS) as m:
        loop = run(m, "far")
    assert shipped is not None and shipped == loop


# ---- grid independence at depth ----
@pytest.mark.parametrize("lanes_log2", [0, 7])
def test_result_does_not_depend_on_the_grid_at_depth(lanes_log2):
    switches = dict(du.FUSED, POW_CHAIN_LANES_LOG2=lanes_log2, POW_BATCH_LANES_LOG2=lanes_log2,
                    POW_RACE_LANES_LOG2=lanes_log2)
    with du.miner_with(**switches) as m:
        chain_row(m, "nines", launches=1)
        batch_row(m, "nines", launches=2)
        race_row(m, "nines", launches=1)
