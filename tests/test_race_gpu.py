"""pow_mine_race on the GPU against its host statement
(mpi_blockchain_amd.block.mine_race, hashlib on the CPU): every comparison is
over all 552 bytes of every block.  The statement never runs the code under
test; d <= 11 and windows of at most 2^16 keep it at a few thousand hashlib
calls per height.  K6 is forced (POW_RACE_FUSED_MAX=32, test library) unless a
test says otherwise."""
import ctypes
import os
import random
import subprocess

import pytest

from mpi_blockchain_amd import _lib
from mpi_blockchain_amd.block import field, make_block, mine_race, nonce_from_counter, set_field
from mpi_blockchain_amd.miner import GpuMiner, StopBoard, refresh_template

import chain_util as cu
import helpers
import race_util as ru

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mpi_blockchain_amd")
SWITCHES = ("POW_RACE_FUSED_MAX", "POW_RACE_BATCH", "POW_RACE_LANES_LOG2", "POW_CHAIN_FUSED_MAX")


def miner_with(**switches):
    """A context of the test library whose pow_init saw the given switches."""
    return helpers.hooked_miner(SWITCHES, **switches)


@pytest.fixture(scope="module")
def fused():
    """K6 at every d <= 32."""
    with miner_with(POW_RACE_FUSED_MAX=32) as m:
        yield m


@pytest.fixture(scope="module")
def shipped():
    """The shipped library, as built."""
    with GpuMiner(0) as m:
        yield m


def check_against_statement(m, parent, n, d, owners, created, start, count, launches=None):
    """The call's bytes, winners, counters and counts against the statement's;
    returns (statement, hashes)."""
    stated = mine_race(parent, n, d, owners, created, start, count)
    k = len(stated[0])
    rc, mined, hashes, winners, ctrs, out = ru.call(m.L, m.ctx, parent, n, d, owners, created, start, count)
    assert rc == (1 if k == n else 0), (rc, m.L.pow_last_error())
    assert mined == k
    want_bytes, want_winners, want_ctrs = ru.expected(stated, n)
    assert winners == want_winners and ctrs == want_ctrs
    assert bytes(out)[:n * ru.BLOCK_BYTES] == want_bytes
    s = m.stats()
    assert s["hashes"] == hashes and s["kernel_ms"] > 0
    # 8: every pair below the answer was tested, and the answer itself
    R = len(owners)
    assert hashes >= sum((c - start) * R + r + 1 for r, c in zip(stated[1], stated[2]))
    if launches is not None:
        assert s["launches"] == launches
    return stated, hashes


# ---- 1: statement parity ----
@pytest.fixture(scope="module")
def two_winner_base():
    """A created_at base whose d = 6 race of three is won from two positions at least."""
    for i in range(64):
        base = 1_700_000_000 + 1000 * i
        if len(set(mine_race(ru.genesis(), 4, 6, [0, 1, 2], ru.times(4, 3, base), 0, 1 << 16)[1])) >= 2:
            return base
    pytest.fail("no created_at base among 64 gives two winning positions")


@pytest.mark.parametrize("d", [0, 1, 6, 11])
def test_statement_parity(fused, two_winner_base, d):
    (blocks, winners, ctrs), _ = check_against_statement(fused, ru.genesis(), 4, d, [0, 1, 2], ru.times(4, 3, two_winner_base),
                                                         0, 1 << 16, launches=4)
    assert len(blocks) == 4
    if d == 0:  # every counter solves: position 0 at ctr_start itself
        assert winners == [0] * 4 and ctrs == [0] * 4
        assert all(field(b, "nonce") == nonce_from_counter(0) and b.node_owner_number == 0 for b in blocks)
    if d == 6:
        assert len(set(winners)) >= 2


# ---- 2: the recorded reference races, the tie included ----
@pytest.mark.parametrize("name", ["three", "tie"])
def test_the_recorded_reference_races(fused, name):
    v, parent, races = ru.fixture()
    r, chain = races[name]
    n = len(chain)
    rc, mined, _, winners, ctrs, out = ru.call(fused.L, fused.ctx, parent, n, v["difficulty"], r["owners"], r["created_at"],
                                               v["ctr_start"], 1 << 16)
    assert (rc, mined) == (1, n), (rc, fused.L.pow_last_error())
    assert (winners, ctrs) == (r["winners"], r["counters"])
    assert bytes(out) == ru.raw(chain)


# ---- 3: ties ----
@pytest.mark.parametrize("owners", [[5, 261], [261, 5], [9, 9, 9]])
def test_ties_go_to_the_lowest_position(fused, owners):
    n, R = 3, len(owners)
    created = [1_700_000_000 + 7 * k for k in range(n) for _ in range(R)]  # equal among the rivals of a height
    (blocks, winners, _), _ = check_against_statement(fused, ru.genesis(), n, 8, owners, created, 0, 1 << 14)
    assert winners == [0] * n
    assert [b.node_owner_number for b in blocks] == [owners[0]] * n


# ---- 4: grid independence ----
@pytest.mark.parametrize("lanes_log2", [0, 7])
def test_result_does_not_depend_on_the_grid(lanes_log2):
    """One workgroup per rival whose lanes walk the window, and as many as the plan allows."""
    with miner_with(POW_RACE_FUSED_MAX=32, POW_RACE_LANES_LOG2=lanes_log2) as m:
        check_against_statement(m, ru.genesis(), 3, 8, [3, 1, 4, 1, 5], ru.times(3, 5), 62 ** 2 - 100, 1 << 14)
        check_against_statement(m, ru.genesis(), 3, 11, [0, 1], ru.times(3, 2), 0, 1 << 16)


# ---- 5: most rivals ----
def test_most_rivals(fused):
    n, R, d, window = 2, 256, 8, 1 << 14
    owners = [(37 * i + 11) % 1000 for i in range(R)]
    created = [1_700_000_000 + 3 * k + (i * i) % 251 for k in range(n) for i in range(R)]
    check_against_statement(fused, ru.genesis(), n, d, owners, created, 0, window, launches=n)
    # (one workgroup per rival: more than one per CU where the card has fewer than 256 CUs)
    rc, mined, hashes, winners, ctrs, out = ru.call(fused.L, fused.ctx, ru.genesis(), n, d, owners + [1], None, 0, window)
    assert rc == _lib.POW_EINVAL and "n_rivals" in (fused.L.pow_last_error() or b"").decode()
    assert (mined, hashes) == (12345, 12345) and bytes(out) == b"\xA5" * (n * ru.BLOCK_BYTES)
    assert winners == [ru.UNSET_WINNER] * n and ctrs == [ru.UNSET_CTR] * n


# ---- 6: a height nobody solves ----
def test_a_height_nobody_solves(fused):
    n, d, window, owners = 5, 10, 700, [0, 1]
    for i in range(64):
        created = ru.times(n, 2, 1_700_000_000 + 1000 * i)
        stated = mine_race(ru.genesis(), n, d, owners, created, 0, window)
        if 1 <= len(stated[0]) <= 3:
            break
    else:
        pytest.fail("no created_at base among 64 stops after 1 to 3 heights")
    k = len(stated[0])
    rc, mined, hashes, winners, ctrs, out = ru.call(fused.L, fused.ctx, ru.genesis(), n, d, owners, created, 0, window)
    assert rc == 0, (rc, fused.L.pow_last_error())
    assert mined == k
    want_bytes, want_winners, want_ctrs = ru.expected(stated, n)
    assert bytes(out) == want_bytes and b"\xA5" * ((n - k) * ru.BLOCK_BYTES) == want_bytes[:(n - k) * ru.BLOCK_BYTES]
    assert winners == want_winners and ctrs == want_ctrs
    # the empty height was searched to its end by both rivals, on top of what the mined heights need
    assert hashes >= window * 2 + sum(c * 2 + r + 1 for r, c in zip(stated[1], stated[2]))
    # ... and the context is as good as before
    check_against_statement(fused, ru.genesis(), 2, 6, owners, ru.times(2, 2), 0, 1 << 12)


# ---- 7: batch boundaries ----
def test_batch_boundaries():
    with miner_with(POW_RACE_FUSED_MAX=32, POW_RACE_BATCH=2) as m:
        created = ru.times(5, 3)
        (five, _, _), _ = check_against_statement(m, ru.genesis(), 5, 6, [0, 1, 2], created, 0, 1 << 16, launches=5)
        (four, _, _), _ = check_against_statement(m, ru.genesis(), 4, 6, [0, 1, 2], created[:12], 0, 1 << 16, launches=4)
        assert ru.raw(five[1:]) == ru.raw(four)


# ---- 9: layout traps ----
def test_layout_traps(fused):
    rng = random.Random(9)
    parent = make_block(0xFFFFFFFF, 3, 9, 1_699_999_990, prev=b"p" * 256, nonce=b"nnnnnnnnnn")
    junk = bytes(rng.randrange(1, 256) for _ in range(256))  # no NUL anywhere, junk behind the hash text too
    set_field(parent, "block_hash", junk)
    ctypes.memset(ctypes.addressof(parent) + 12, 0xEE, 4)   # the padding behind difficulty ...
    ctypes.memset(ctypes.addressof(parent) + 546, 0xDD, 6)  # ... and behind block_hash
    owners = [0x1FF, 0x2FE, 7]
    created = [(1 << 40) + 5 + 11 * k + 3 * r for k in range(3) for r in range(3)]
    (blocks, winners, _), _ = check_against_statement(fused, parent, 3, 6, owners, created, 0, 1 << 16)
    oldest = ru.raw(blocks[-1:])
    assert blocks[-1].index == 0 and blocks[0].index == 2  # index + 1 wraps
    assert oldest[34:290] == junk and oldest[290 + 65:546] == junk[65:]
    for b, w in zip(blocks, winners):
        r = ru.raw([b])
        assert r[12:16] == b"\xEE" * 4 and r[546:] == b"\xDD" * 6 and r[33] == 0 and r[290 + 64] == 0
        assert b.node_owner_number == owners[w] and b.created_at > 1 << 40


# ---- 10: counter edges ----
@pytest.mark.parametrize("start", [62 ** 4 - 3, 62 ** 6 - 3, 62 ** 7 - 3, 62 ** 8 - 3, 62 ** 9 - (1 << 12)])
def test_counter_edges(fused, start):
    check_against_statement(fused, ru.genesis(), 3, 4, [2, 0, 1], ru.times(3, 3), start, 1 << 12)


# ---- 11: the paths agree ----
def test_paths_agree(shipped):
    n, d, window, owners = 3, 14, 1 << 24, [0, 1, 2, 3, 4, 5]
    R = len(owners)
    created = ru.times(n, R)
    results = {}
    rc, mined, _, winners, ctrs, out = ru.call(shipped.L, shipped.ctx, ru.genesis(), n, d, owners, created, 0, window)
    assert (rc, mined) == (1, n), (rc, shipped.L.pow_last_error())
    results["shipped"] = (winners, ctrs, bytes(out))
    with miner_with(POW_RACE_FUSED_MAX=-1) as h:
        rc, mined, _, winners, ctrs, out = ru.call(h.L, h.ctx, ru.genesis(), n, d, owners, created, 0, window)
        assert (rc, mined) == (1, n) and h.stats()["launches"] >= n
        results["loop"] = (winners, ctrs, bytes(out))
    with miner_with(POW_RACE_FUSED_MAX=32) as f:  # K6 whatever the built threshold is
        rc, mined, hashes, winners, ctrs, out = ru.call(f.L, f.ctx, ru.genesis(), n, d, owners, created, 0, window)
        assert (rc, mined) == (1, n) and f.stats()["launches"] == n
        assert hashes >= sum(c * R + r + 1 for r, c in zip(winners, ctrs))
        results["fused"] = (winners, ctrs, bytes(out))
        # one rival is pow_mine_chain, on the fused library too
        one = [created[k * R] for k in range(n)]
        rc, mined, _, w1, c1, o1 = ru.call(f.L, f.ctx, ru.genesis(), n, d, owners[:1], one, 0, window)
        rcc, minedc, _, oc = cu.call(f.L, f.ctx, ru.genesis(), n, d, owners[0], one, 0, window)
        assert (rc, mined, w1) == (rcc, minedc, [0] * n) == (1, n, [0] * n) and bytes(o1) == bytes(oc)
        assert [nonce_from_counter(c) for c in c1] == [field(b, "nonce") for b in o1]
    assert results["shipped"] == results["loop"] == results["fused"]
    # the loop of examples/mine_race.c by hand: refresh, pow_mine_batch, the lowest (counter, position)
    last, by_hand = ru.genesis(), []
    for k in range(n):
        tmpls = [refresh_template(last, owners[r], d, created[k * R + r]) for r in range(R)]
        b = shipped.mine_batch(tmpls, d, 0, window)
        assert b.complete
        c, r = min((c, r) for r, c in enumerate(b.counters))
        by_hand.insert(0, (r, c, b.blocks[r]))
        last = b.blocks[r]
    assert ([r for r, _, _ in by_hand], [c for _, c, _ in by_hand], ru.raw([b for _, _, b in by_hand])) == results["fused"]


def test_host_loop_against_the_statement():
    """The loop's own corners: ctr_start itself solves (nothing lies below it for
    the later rivals), ties, and a height nobody solves."""
    with miner_with(POW_RACE_FUSED_MAX=-1) as h:
        (_, winners, ctrs), _ = check_against_statement(h, ru.genesis(), 3, 0, [3, 4], ru.times(3, 2), 62 ** 4 - 3, 5)
        assert winners == [0] * 3 and ctrs == [62 ** 4 - 3] * 3
        equal = [1_700_000_000 + 7 * k for k in range(3) for _ in range(3)]
        (_, winners, _), _ = check_against_statement(h, ru.genesis(), 3, 6, [5, 261, 9], equal, 0, 1 << 12)
        assert 1 not in winners  # 261 never beats 5
        (blocks, _, _), hashes = check_against_statement(h, ru.genesis(), 4, 12, [0, 1], ru.times(4, 2), 0, 8)
        assert len(blocks) < 4 and hashes >= 16


# ---- 12: the audit ----
def test_result_passes_the_audit(fused):
    n, d, owners = 6, 9, [4, 5, 6]
    parent = ru.genesis()
    r = fused.mine_race(parent, n, d, owners, ru.times(n, 3), 0, 1 << 16)
    assert r.complete and r.n_mined == n
    chain = (_lib.Block * (n + 1))()
    ctypes.memmove(chain, r.blocks, n * ru.BLOCK_BYTES)
    ctypes.memmove(ctypes.byref(chain, n * ru.BLOCK_BYTES), ctypes.addressof(parent), ru.BLOCK_BYTES)
    v = fused.verify_chain(chain, d)
    # the parent is the genesis block: its own hash and work are not the race's (node.cpp:361-372)
    assert v.status[:n].tolist() == [0] * n and v.first_bad >= n


# ---- 13: early outs ----
def test_nothing_to_mine(fused):
    rc, mined, hashes, winners, ctrs, out = ru.call(fused.L, fused.ctx, ru.genesis(), 0, 6, [0, 1], None, 0, 1 << 16)
    assert (rc, mined, hashes, winners, ctrs) == (1, 0, 0, [], [])
    assert bytes(out) == b"\xA5" * ru.BLOCK_BYTES
    assert fused.stats()["launches"] == 0


def test_cancel_word_moved_at_entry(fused):
    rc, mined, hashes, winners, ctrs, out = ru.call(fused.L, fused.ctx, ru.genesis(), 3, 6, [0, 1], None, 0, 1 << 16,
                                                    cancel=ctypes.byref(ctypes.c_uint32(8)), epoch=7)
    assert (rc, mined, hashes) == (0, 0, 0)
    assert fused.stats()["launches"] == 0
    assert bytes(out) == b"\xA5" * (3 * ru.BLOCK_BYTES)
    assert winners == [ru.UNSET_WINNER] * 3 and ctrs == [ru.UNSET_CTR] * 3


def test_board_bound_context_is_refused():
    with miner_with(POW_RACE_FUSED_MAX=32) as m, StopBoard(2) as board:
        m.bind_board(board, 0, 1)
        try:
            rc, mined, hashes, winners, ctrs, out = ru.call(m.L, m.ctx, ru.genesis(), 2, 6, [0, 1], None, 0, 1 << 16)
            assert rc == _lib.POW_EINVAL and (mined, hashes) == (12345, 12345)
            assert "board" in (m.L.pow_last_error() or b"").decode()
            assert bytes(out) == b"\xA5" * (2 * ru.BLOCK_BYTES) and winners == [ru.UNSET_WINNER] * 2
        finally:
            m.bind_board(None)
        check_against_statement(m, ru.genesis(), 2, 6, [0, 1], ru.times(2, 2), 0, 1 << 16)


# ---- 14: the Python wrapper and the C example ----
def test_python_wrapper(fused):
    n, d, owners = 4, 8, [0, 1, 2]
    created = ru.times(n, 3)
    blocks, winners, ctrs = mine_race(ru.genesis(), n, d, owners, created, 0, 1 << 14)
    r = fused.mine_race(ru.genesis(), n, d, owners, created, 0, 1 << 14)
    assert r.complete and r.n_mined == n == len(r.blocks) and r.hashes > 0 and r.kernel_ms > 0
    assert (r.winners, r.counters) == (winners, ctrs) and ru.raw(r.blocks) == ru.raw(blocks)
    short = fused.mine_race(ru.genesis(), 3, 12, [0, 1], ru.times(3, 2), 0, 8)  # 16 trials at d = 12: next to hopeless
    stated = mine_race(ru.genesis(), 3, 12, [0, 1], ru.times(3, 2), 0, 8)
    assert not short.complete and short.n_mined == len(stated[0]) == len(short.winners) == len(short.counters)
    with pytest.raises(ValueError):
        fused.mine_race(ru.genesis(), 2, 6, [0, 1], [1, 2, 3])


def test_c_example(tmp_path):
    exe = str(tmp_path / "mine_race_fused")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "mine_race_fused.c"), "-L", PKG, "-lpow_gpu",
                    f"-Wl,-rpath,{PKG}", "-o", exe], check=True)
    p = subprocess.run([exe, "4", "5", "9"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "chain of 5 blocks at difficulty 9: valid" in p.stdout
    assert p.stdout.count("\nblock ") + p.stdout.startswith("block ") == 5
    assert "4 miners, " in p.stdout
