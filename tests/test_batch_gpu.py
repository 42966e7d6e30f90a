"""pow_mine_batch on the GPU against its host statement
(mpi_blockchain_amd.block.mine_batch, hashlib on the CPU): every comparison is
over all 552 bytes of every block.  The statement never runs the code under
test; d <= 11 keeps it at a few thousand hashlib calls per template.  K5 is
forced (POW_BATCH_FUSED_MAX=32, test library) unless a test says otherwise."""
import ctypes
import os
import random
import subprocess

import pytest

from mpi_blockchain_amd import _lib
from mpi_blockchain_amd.block import field, make_block, mine_batch, nonce_from_counter, set_field
from mpi_blockchain_amd.miner import GpuMiner, StopBoard

import batch_util as bu
import helpers

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mpi_blockchain_amd")
SWITCHES = ("POW_BATCH_FUSED_MAX", "POW_BATCH_TILE", "POW_BATCH_LANES_LOG2")


def miner_with(**switches):
    """A context of the test library whose pow_init saw the given switches."""
    return helpers.hooked_miner(SWITCHES, **switches)


@pytest.fixture(scope="module")
def fused():
    """K5 at every d <= 32."""
    with miner_with(POW_BATCH_FUSED_MAX=32) as m:
        yield m


@pytest.fixture(scope="module")
def shipped():
    """The shipped library, as built."""
    with GpuMiner(0) as m:
        yield m


def mixed_templates(n=5):
    """Templates that differ in owner, created_at, index and previous hash."""
    rng = random.Random(5)
    return [make_block(1 + 3 * i, 10 + i, 9, 1_700_000_000 + 13 * i + (i * i) % 7,
                       prev=bytes(rng.choice(b"0123456789abcdef") for _ in range(64))) for i in range(n)]


def check_against_statement(m, tmpls, d, start, count, launches=None, in_place=False):
    stated = mine_batch(tmpls, d, start, count)
    k = sum(b is not None for b, _ in stated)
    rc, solved, hashes, ctrs, out = bu.call(m.L, m.ctx, tmpls, d, start, count, in_place=in_place)
    assert rc == (1 if k == len(tmpls) else 0), (rc, m.L.pow_last_error())
    assert solved == k
    assert ctrs == [c if c is not None else bu.NONE for _, c in stated]
    if in_place:
        want = b"".join(bu.raw([b if b is not None else t]) for (b, _), t in zip(stated, tmpls))
    else:
        want = bu.expected_bytes(stated)
    assert bytes(out)[:len(want)] == want
    s = m.stats()
    assert s["hashes"] == hashes and hashes >= len(tmpls) and s["kernel_ms"] > 0
    if launches is not None:
        assert s["launches"] == launches
    return stated


# ---- 1: statement parity ----
@pytest.mark.parametrize("d", [0, 1, 6, 11])
def test_statement_parity(fused, d):
    stated = check_against_statement(fused, mixed_templates(), d, 0, 1 << 16, launches=1)
    assert all(b is not None for b, _ in stated)
    if d == 0:  # every counter solves: the lowest is ctr_start itself
        assert all(c == 0 and field(b, "nonce") == nonce_from_counter(0) for b, c in stated)


def test_the_recorded_reference_batch(fused):
    v, tmpls, sealed = bu.fixture()
    rc, solved, _, ctrs, out = bu.call(fused.L, fused.ctx, tmpls, v["difficulty"], 0, 1 << 16)
    assert (rc, solved) == (1, 6) and ctrs == v["counters"]
    assert bytes(out) == bu.raw(sealed)


# ---- 2: grid independence ----
@pytest.mark.parametrize("lanes_log2", [0, 7])
def test_result_does_not_depend_on_the_grid(lanes_log2):
    """One workgroup per template whose lanes walk the window (d = 8 at 2^0 x 256
    lanes: most templates need several strides) and as many as the plan allows."""
    with miner_with(POW_BATCH_FUSED_MAX=32, POW_BATCH_LANES_LOG2=lanes_log2) as m:
        check_against_statement(m, mixed_templates(), 8, 62 ** 2 - 100, 1 << 14)
        check_against_statement(m, mixed_templates(3), 11, 0, 1 << 16)


# ---- 3: tile boundaries ----
def test_nine_templates_in_tiles_of_four():
    with miner_with(POW_BATCH_FUSED_MAX=32, POW_BATCH_TILE=4) as m:
        tmpls = bu.race_templates(9, 6)
        check_against_statement(m, tmpls, 6, 0, 1 << 16, launches=3)
        check_against_statement(m, tmpls[:8], 6, 0, 1 << 16, launches=2)


# ---- 4: solved and unsolved mixed ----
def test_solved_and_unsolved_mixed(fused):
    n, d, window = 8, 10, 700
    for base in range(1_700_000_000, 1_700_000_000 + 64 * 1000, 1000):
        tmpls = bu.race_templates(n, d, base)
        stated = mine_batch(tmpls, d, 0, window)
        k = sum(b is not None for b, _ in stated)
        if 2 <= k <= 6:
            break
    else:
        pytest.fail("no created_at base solves between 2 and 6 of the 8 templates")
    rc, solved, hashes, ctrs, out = bu.call(fused.L, fused.ctx, tmpls, d, 0, window)
    assert rc == 0, (rc, fused.L.pow_last_error())
    assert solved == k
    assert bytes(out) == bu.expected_bytes(stated)  # unsolved entries are still the 0xA5 fill
    assert ctrs == [c if c is not None else bu.NONE for _, c in stated]
    assert hashes >= window * (n - k)  # every empty window was searched to its end
    assert fused.stats()["launches"] == 1


# ---- 5: more workgroups than the chip holds ----
def test_more_workgroups_than_the_chip_holds():
    n, d, window = 1500, 8, 1 << 14
    tmpls = [make_block(1 + i // 256, i, d, 1_700_000_000 + i) for i in range(n)]
    stated = mine_batch(tmpls, d, 0, window)
    assert all(b is not None for b, _ in stated)
    # four times the expected trials in lanes, whatever the plan would pick: 4 workgroups per template
    with miner_with(POW_BATCH_FUSED_MAX=32, POW_BATCH_LANES_LOG2=2) as m:
        rc, solved, hashes, ctrs, out = bu.call(m.L, m.ctx, tmpls, d, 0, window)
        assert rc == 1, (rc, m.L.pow_last_error())
        assert solved == n and ctrs == [c for _, c in stated]
        assert bytes(out) == bu.expected_bytes(stated)
        assert 4 * n > 8 * m.device_info()["cu_count"]  # 6,000 workgroups: several times what is resident at once
        # one launch, and every workgroup of it ran at least its first stride or saw a published hit
        assert m.stats()["launches"] == 1 and hashes >= sum(c + 1 for _, c in stated)
    # ... and the plan's own grid (one workgroup per template here) gives the same bytes
    with miner_with(POW_BATCH_FUSED_MAX=32) as m:
        rc, solved, _, ctrs, out = bu.call(m.L, m.ctx, tmpls, d, 0, window)
        assert (rc, solved) == (1, n) and bytes(out) == bu.expected_bytes(stated)


# ---- 6: layout traps ----
def trap_template(index, seed):
    rng = random.Random(seed)
    t = make_block(index, 0x1FF, 3, (1 << 40) + 5 + seed, nonce=b"nnnnnnnnnn",
                   prev=bytes(rng.randrange(1, 256) for _ in range(256)))  # no NUL anywhere
    set_field(t, "block_hash", bytes(rng.randrange(1, 256) for _ in range(256)))  # junk, also behind byte 64
    ctypes.memset(ctypes.addressof(t) + 12, 0xEE, 4)   # the padding behind difficulty ...
    ctypes.memset(ctypes.addressof(t) + 546, 0xDD, 6)  # ... and behind block_hash
    return t


def test_layout_traps(fused):
    tmpls = [trap_template(0x1FE, 1), trap_template(0xFFFFFFFF, 2), trap_template(7, 3)]
    stated = check_against_statement(fused, tmpls, 6, 0, 1 << 16)
    for (b, _), t in zip(stated, tmpls):
        r, tr = bu.raw([b]), bu.raw([t])
        assert r[12:16] == b"\xEE" * 4 and r[546:] == b"\xDD" * 6
        assert r[34:290] == tr[34:290] and b"\0" not in r[34:290]
        assert r[290 + 65:546] == tr[290 + 65:546] and r[33] == 0 and r[290 + 64] == 0


# ---- 7: counter edges ----
@pytest.mark.parametrize("start", [62 ** 4 - 3, 62 ** 6 - 3, 62 ** 7 - 3, 62 ** 8 - 3, 62 ** 9 - (1 << 12)])
def test_counter_edges(fused, start):
    check_against_statement(fused, mixed_templates(3), 4, start, 1 << 12)


# ---- 8: no cross-talk ----
def test_no_cross_talk(fused):
    t = mixed_templates(1)[0]
    stated = check_against_statement(fused, [t, t, t], 8, 0, 1 << 14)
    assert len({bu.raw([b]) for b, _ in stated}) == 1
    a = make_block(1, 0, 9, 1_700_000_000, prev=b"a" * 255 + b"x")
    b = make_block(1, 0, 9, 1_700_000_000, prev=b"a" * 255 + b"y")  # differs in previous_block_hash[255] only
    (sa, _), (sb, _) = check_against_statement(fused, [a, b], 8, 0, 1 << 14)
    assert field(sa, "block_hash")[:64] != field(sb, "block_hash")[:64]


# ---- 9: in place ----
def test_in_place(fused):
    tmpls = mixed_templates()
    check_against_statement(fused, tmpls, 8, 0, 1 << 14, in_place=True)
    # ... with an unsolved template, which then stays as it was
    check_against_statement(fused, bu.race_templates(8, 10), 10, 0, 700, in_place=True)


# ---- 10: the three paths agree ----
def test_three_paths_agree(shipped):
    n, d, window = 6, 14, 1 << 24
    tmpls = bu.race_templates(n, d)
    results = {}
    rc, solved, _, ctrs, out = bu.call(shipped.L, shipped.ctx, tmpls, d, 0, window)
    assert (rc, solved) == (1, n), (rc, shipped.L.pow_last_error())
    results["shipped"] = (ctrs, bytes(out))
    with miner_with(POW_BATCH_FUSED_MAX=-1) as h:
        rc, solved, _, ctrs, out = bu.call(h.L, h.ctx, tmpls, d, 0, window)
        assert (rc, solved) == (1, n) and h.stats()["launches"] >= n
        results["loop"] = (ctrs, bytes(out))
    with miner_with(POW_BATCH_FUSED_MAX=32) as f:  # K5 whatever the built threshold is
        rc, solved, _, ctrs, out = bu.call(f.L, f.ctx, tmpls, d, 0, window)
        assert (rc, solved) == (1, n)
        tile = min((1 << 26) >> d, (1 << 38) // window, 1 << 14)  # the plan; the grid cap is far off
        assert f.stats()["launches"] == -(-n // tile) == 1
        results["fused"] = (ctrs, bytes(out))
        # n == 1 is pow_mine itself, on the fused library too
        rc, solved, _, c1, o1 = bu.call(f.L, f.ctx, tmpls[:1], d, 0, window)
        assert (rc, solved, c1) == (1, 1, results["fused"][0][:1]) and bytes(o1) == results["fused"][1][:bu.BLOCK_BYTES]
    assert results["shipped"] == results["loop"] == results["fused"]
    by_hand = [shipped.mine(t, 0, window, d) for t in tmpls]
    assert all(r is not None for r in by_hand)
    assert [r.counter for r in by_hand] == results["fused"][0]
    assert bu.raw([r.block for r in by_hand]) == results["fused"][1]


# ---- 11: early outs ----
def test_nothing_to_mine(fused):
    rc, solved, hashes, ctrs, out = bu.call(fused.L, fused.ctx, [], 6, 0, 1 << 16)
    assert (rc, solved, hashes, ctrs) == (1, 0, 0, [])
    assert bytes(out) == b"\xA5" * bu.BLOCK_BYTES
    assert fused.stats()["launches"] == 0


def test_cancel_word_moved_at_entry(fused):
    tmpls = mixed_templates()
    rc, solved, hashes, ctrs, out = bu.call(fused.L, fused.ctx, tmpls, 6, 0, 1 << 16,
                                            cancel=ctypes.byref(ctypes.c_uint32(8)), epoch=7)
    assert (rc, solved, hashes) == (0, 0, 0)
    assert fused.stats()["launches"] == 0
    assert bytes(out) == b"\xA5" * (5 * bu.BLOCK_BYTES)
    assert ctrs == [bu.NONE] * 5


def test_board_bound_context_is_refused():
    with miner_with(POW_BATCH_FUSED_MAX=32) as m, StopBoard(2) as board:
        m.bind_board(board, 0, 1)
        try:
            rc, solved, _, ctrs, out = bu.call(m.L, m.ctx, mixed_templates(2), 6, 0, 1 << 16)
            assert rc == _lib.POW_EINVAL and solved == 12345 and ctrs == [12345, 12345]
            assert "board" in (m.L.pow_last_error() or b"").decode()
            assert bytes(out) == b"\xA5" * (2 * bu.BLOCK_BYTES)
        finally:
            m.bind_board(None)
        check_against_statement(m, mixed_templates(2), 6, 0, 1 << 16)


def test_python_wrapper(fused):
    tmpls = bu.race_templates(8, 10)
    stated = mine_batch(tmpls, 10, 0, 700)
    r = fused.mine_batch(tmpls, 10, 0, 700)
    assert r.counters == [c for _, c in stated] and r.n_solved == sum(c is not None for c in r.counters)
    assert not r.complete and r.hashes > 0 and r.kernel_ms > 0
    assert [b is None for b in r.blocks] == [b is None for b, _ in stated]
    assert bu.raw([b for b in r.blocks if b is not None]) == bu.raw([b for b, _ in stated if b is not None])


# ---- 12: the C example ----
def test_c_example(tmp_path):
    exe = str(tmp_path / "mine_race")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "mine_race.c"), "-L", PKG, "-lpow_gpu",
                    f"-Wl,-rpath,{PKG}", "-o", exe], check=True)
    p = subprocess.run([exe, "4", "5", "9"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "chain of 5 blocks at difficulty 9: valid" in p.stdout
    assert p.stdout.count("\nblock ") + p.stdout.startswith("block ") == 5
