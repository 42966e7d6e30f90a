"""pow_mine_rand (K8) on the GPU: the reference's own blocks from its own seeds
(tests/golden/rand_replay.json, made by the reference's code), and the lowest
solving trial against a brute force over tests/rand_util.py and hashlib, which
never runs the code under test.  Every comparison of a block is over all 552
bytes.  The shapes are the smallest at which K8 can still go wrong: d <= 15
keeps the brute force at tens of thousands of hashlib calls."""
import ctypes
import functools
import json
import os
import subprocess

import pytest

import rand_util
from mpi_blockchain_amd import _lib
from mpi_blockchain_amd.miner import GpuMiner, StopBoard, rand_nonces, refresh_template, replay_proof_of_work

from helpers import block_from_template
from rand_gpu_util import SEED, block_of, brute, call, check_against_brute, miner_with, raw

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mpi_blockchain_amd")
LIMIT = 1 << 56


@pytest.fixture(scope="module")
def shipped():
    """The shipped library, as built: the default plan."""
    with GpuMiner(0) as m:
        yield m


@pytest.fixture(scope="module")
def replay():
    with open(os.path.join(ROOT, "tests", "golden", "rand_replay.json")) as f:
        return json.load(f)


# ---- 1: the headline ----
def test_replay_reproduces_the_reference_s_blocks(shipped, replay):
    """Every recorded replay of the reference byte for byte: the 552 bytes of
    each of the 3 blocks, the trial each solved at, and the total trials."""
    assert len(replay["replays"]) >= 5 and {r["template"] for r in replay["replays"]} >= {"S0", "S1", "S2"}
    for r in replay["replays"]:
        parent = block_of(bytes.fromhex(r["parent_hex"]))
        blocks, total = replay_proof_of_work(shipped, parent, r["rank"], r["seed"], len(r["blocks"]), r["difficulty"],
                                             r["created_at"])
        assert [raw(b).hex() for b in blocks] == [b["block_hex"] for b in r["blocks"]], (r["seed"], r["template"])
        assert total == r["total_trials"] == r["blocks"][-1]["trial"] + 1
        # the trial of each block, by mining it again from where the stream stood
        at, last = 0, parent
        for k, want in enumerate(r["blocks"]):
            hit = shipped.mine_rand(refresh_template(last, r["rank"], r["difficulty"], r["created_at"][k]), r["seed"], at,
                                    1 << 32, r["difficulty"])
            assert hit is not None and hit.trial == want["trial"] and raw(hit.block).hex() == want["block_hex"]
            assert hit.hashes >= hit.trial - at + 1
            at, last = hit.trial + 1, hit.block


# ---- 2: the lowest trial against brute force ----
# 1234577 is a multiple of neither 31 nor 9; the last window ends exactly at POW_RAND_TRIAL_LIMIT
STARTS = {"zero": (0, 1 << 20), "odd": (1234577, 1 << 20), "deep": ((1 << 40) + 123, 1 << 20),
          "limit": (LIMIT - (1 << 17), 1 << 17)}
assert 1234577 % 31 and 1234577 % 9


@pytest.mark.parametrize("where", list(STARTS))
@pytest.mark.parametrize("name", ["S0", "S2"])
def test_lowest_trial_against_brute_force(shipped, templates, name, where):
    start, count = STARTS[where]
    tmpl = block_from_template(templates[name])
    for d in (0, 1, 9, 13):
        trial = check_against_brute(shipped, tmpl, SEED, start, count, d)
        assert trial is not None and (d > 0 or trial == start)


# ---- 3: window edges ----
def test_window_edges(shipped, templates):
    tmpl = block_from_template(templates["S2"])
    start = 1234577
    (found, nonce, hexd), = brute(raw(tmpl), SEED, start, 1 << 20, 9)
    assert found > start
    # the answer is the last trial of the window
    assert check_against_brute(shipped, tmpl, SEED, start, found - start + 1, 9) == found
    # one shorter: nothing, and out untouched
    assert check_against_brute(shipped, tmpl, SEED, start, found - start, 9) is None
    # count = 1: on the answer, and next to it
    assert check_against_brute(shipped, tmpl, SEED, found, 1, 9) == found
    assert check_against_brute(shipped, tmpl, SEED, found - 1, 1, 9) is None
    # in place: out = tmpl
    t2 = block_of(raw(tmpl))
    assert shipped.L.pow_mine_rand(shipped.ctx, ctypes.byref(t2), SEED, start, 1 << 20, 9, None, 0, ctypes.byref(t2),
                                   None, None) == 1
    assert raw(t2) == rand_util.seal(raw(tmpl), nonce, hexd)


# ---- 4: forced shapes through the test library ----
@functools.lru_cache(maxsize=None)
def far_case(tmpl_bytes: bytes):
    """A window at d = 15 whose answer lies at least 2^15 trials in: past the
    first pass of every forced shape below (at most 512 lanes x 64), and in
    launch 32 or later of 2^10-trial launches."""
    for start in range(5000, 5000 + 64 * 100003, 100003):
        if not brute(tmpl_bytes, SEED, start, 1 << 15, 15):
            hits = brute(tmpl_bytes, SEED, start, 1 << 19, 15)
            if hits:
                return start, hits[0]
    raise AssertionError("no such window")


@pytest.mark.parametrize("lanes_log2", [8, 9])  # one and two workgroups
@pytest.mark.parametrize("run", [1, 4, 64])
def test_forced_run_and_grid(shipped, templates, run, lanes_log2):
    tmpl = block_from_template(templates["S2"])
    start, (trial, nonce, hexd) = far_case(raw(tmpl))
    assert trial - start >= (1 << lanes_log2) * run  # the answer lies in pass 2 or later
    with miner_with(POW_RAND_RUN=run, POW_RAND_LANES_LOG2=lanes_log2) as m:
        got = call(m, tmpl, SEED, start, 1 << 19, 15)
        assert m.stats()["launches"] == 1
    assert got[:3] == (1, rand_util.seal(raw(tmpl), nonce, hexd), trial)
    assert got[:3] == call(shipped, tmpl, SEED, start, 1 << 19, 15)[:3]  # the default plan


def test_forced_small_launches(shipped, templates):
    tmpl = block_from_template(templates["S2"])
    start, (trial, nonce, hexd) = far_case(raw(tmpl))
    with miner_with(POW_RAND_LAUNCH_LOG2=10) as m:
        got = call(m, tmpl, SEED, start, 1 << 19, 15)
        assert m.stats()["launches"] == (trial - start) // 1024 + 1 >= 3
    assert got[:3] == (1, rand_util.seal(raw(tmpl), nonce, hexd), trial)
    assert got[:3] == call(shipped, tmpl, SEED, start, 1 << 19, 15)[:3]
    assert got[3] >= trial - start + 1


# ---- 5: order independence ----
@functools.lru_cache(maxsize=None)
def close_pair(tmpl_bytes: bytes):
    """Two solutions at d = 6 at most 2 trials apart, and the solution before them."""
    hits = brute(tmpl_bytes, SEED, 0, 1 << 15, 6, 1 << 15)
    for prev, lo, hi in zip(hits, hits[1:], hits[2:]):
        if hi[0] - lo[0] <= 2:
            return prev[0], lo, hi
    raise AssertionError("no close pair")


@pytest.mark.parametrize("shape", [dict(), dict(POW_RAND_LANES_LOG2=8), dict(POW_RAND_LANES_LOG2=10, POW_RAND_RUN=2),
                                   dict(POW_RAND_LANES_LOG2=9, POW_RAND_RUN=16)])
def test_the_lower_of_two_close_solutions_wins(templates, shape):
    tmpl = block_from_template(templates["S0"])
    prev, lo, hi = close_pair(raw(tmpl))
    with miner_with(**shape) as m:
        for start, want in ((prev + 1, lo), (max(prev + 1, lo[0] - 300), lo), (lo[0], lo), (lo[0] + 1, hi)):
            rc, out, found, _ = call(m, tmpl, SEED, start, 1 << 15, 6)
            assert (rc, found) == (1, want[0]), (shape, start)
            assert out == rand_util.seal(raw(tmpl), want[1], want[2])


# ---- 6: cancel, board, null pointers ----
def test_cancel_word_moved_at_entry(shipped, templates):
    tmpl = block_from_template(templates["S0"])
    assert call(shipped, tmpl, SEED, 0, 1 << 20, 9)[0] == 1 and shipped.stats()["launches"] == 1
    rc, out, found, hashes = call(shipped, tmpl, SEED, 0, 1 << 20, 9, cancel=ctypes.byref(ctypes.c_uint32(8)), epoch=7)
    assert (rc, out, found, hashes) == (0, b"\xA5" * 552, 12345, 0)
    assert shipped.stats()["launches"] == 0
    # a word that equals the epoch does not cancel
    assert call(shipped, tmpl, SEED, 0, 1 << 20, 9, cancel=ctypes.byref(ctypes.c_uint32(7)), epoch=7)[0] == 1


def test_board_bound_context_and_null_pointers_are_refused(templates):
    tmpl = block_from_template(templates["S0"])
    with GpuMiner(0) as m, StopBoard(2) as board:
        out = _lib.Block()
        for t, o in ((None, ctypes.byref(out)), (ctypes.byref(tmpl), None)):
            assert m.L.pow_mine_rand(m.ctx, t, SEED, 0, 1 << 20, 9, None, 0, o, None, None) == _lib.POW_EINVAL
            assert "null" in (m.L.pow_last_error() or b"").decode()
        m.bind_board(board, 0, 1)
        try:
            rc, got, found, hashes = call(m, tmpl, SEED, 0, 1 << 20, 9)
            assert rc == _lib.POW_EINVAL and (got, found, hashes) == (b"\xA5" * 552, 12345, 12345)
            assert "board" in (m.L.pow_last_error() or b"").decode()
            # the range check comes before the null check, the null check before the board
            assert m.L.pow_mine_rand(m.ctx, None, SEED, LIMIT, 1, 9, None, 0, None, None, None) == _lib.POW_EINVAL
            assert "LIMIT" in (m.L.pow_last_error() or b"").decode()
            assert m.L.pow_mine_rand(m.ctx, None, SEED, 0, 1, 9, None, 0, None, None, None) == _lib.POW_EINVAL
            assert "null" in (m.L.pow_last_error() or b"").decode()
        finally:
            m.bind_board(None)
        assert check_against_brute(m, tmpl, SEED, 0, 1 << 20, 9) is not None


# ---- 7: stats and the Python mirror ----
def test_stats_and_python_wrapper(shipped, templates):
    tmpl = block_from_template(templates["S1"])
    (trial, nonce, hexd), = brute(raw(tmpl), SEED, 77, 1 << 20, 9)
    r = shipped.mine_rand(tmpl, SEED, 77, 1 << 20, 9)
    s = shipped.stats()
    assert r is not None and r.trial == trial and raw(r.block) == rand_util.seal(raw(tmpl), nonce, hexd)
    assert r.block.nonce == rand_nonces(SEED, trial)[0][:9]
    assert s["launches"] == 1 and s["kernel_ms"] > 0 and r.kernel_ms == s["kernel_ms"]
    # at least the trials up to the answer; at most the window's: a lane goes on until it sees a
    # published hit, so lanes of a later pass may have run, but no trial is tested twice
    assert trial - 77 + 1 <= r.hashes == s["hashes"] <= 1 << 20
    assert shipped.mine_rand(tmpl, SEED, 77, trial - 77, 9) is None


# ---- 8: the C example ----
def test_c_example(tmp_path, replay):
    exe = str(tmp_path / "mine_rand")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "mine_rand.c"), "-L", PKG, "-lpow_gpu",
                    f"-Wl,-rpath,{PKG}", "-o", exe], check=True)
    r = replay["replays"][0]  # seed 0 on S0's parent, the block the example starts from, with its created_at
    assert (r["seed"], r["template"], r["rank"], r["created_at"][0]) == (0, "S0", 0, 1700000000)
    p = subprocess.run([exe, "0", "3", "9"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "chain of 3 blocks at difficulty 9: valid" in p.stdout
    lines = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("block ")]
    assert [(int(ln[3]), ln[7]) for ln in lines] == \
        [(b["trial"], bytes.fromhex(b["block_hex"])[290:354].decode()) for b in r["blocks"]]
    assert f"{r['total_trials']} trials" in p.stdout
