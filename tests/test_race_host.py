"""pow_mine_race on the host (CPU only): its statement
mpi_blockchain_amd.block.mine_race against two races mined through the
reference's own block_to_hash and solves_problem
(tests/golden/mined_race.json) and against the composition it stands for, the
argument errors of the C entry point, which need no GPU, and the fused path's
pure plan (csrc/pow_host.cpp) under sanitizers in a process of its own."""
import ctypes
import os
import subprocess

import pytest

from mpi_blockchain_amd import _lib
from mpi_blockchain_amd.block import field, make_block, mine_batch, mine_chain, mine_race, nonce_from_counter, verify_chain
from mpi_blockchain_amd.miner import refresh_template

import race_util as ru

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpi_blockchain_amd", "csrc")


@pytest.fixture(scope="module")
def recorded():
    return ru.fixture()


@pytest.mark.parametrize("name", ["three", "tie"])
def test_statement_gives_the_recorded_races(recorded, name):
    v, parent, races = recorded
    r, chain = races[name]
    n, R = len(chain), len(r["owners"])
    assert v["difficulty"] == 8 and len(r["created_at"]) == n * R
    blocks, winners, counters = mine_race(parent, n, v["difficulty"], r["owners"], r["created_at"], v["ctr_start"], 1 << 16)
    assert (winners, counters) == (r["winners"], r["counters"])
    assert ru.raw(blocks) == ru.raw(chain)
    for b, w, c in zip(chain, winners, counters):
        assert b.node_owner_number == r["owners"][w] and field(b, "nonce") == nonce_from_counter(c)
    assert verify_chain(chain + [parent], v["difficulty"])[:n] == [0] * n
    if name == "three":
        assert (n, r["owners"]) == (4, [0, 1, 2]) and len(set(winners)) >= 2
    else:  # equal digests at every counter: position 0 wins, and its owner is in the block
        assert (n, r["owners"]) == (2, [7, 263]) and winners == [0, 0]
        assert r["created_at"][0] == r["created_at"][1] and r["created_at"][2] == r["created_at"][3]
        assert [b.node_owner_number for b in chain] == [7, 7]
        swapped = mine_race(parent, n, v["difficulty"], [263, 7], r["created_at"], 0, 1 << 16)
        assert swapped[1:] == (winners, counters) and [b.node_owner_number for b in swapped[0]] == [263, 263]


def by_composition(parent, n, d, owners, created_at, start, count):
    """Refresh, block.mine_batch, the lowest (counter, position), the next height."""
    R = len(owners)
    blocks, winners, counters = [], [], []
    last = parent
    for k in range(n):
        tmpls = [refresh_template(last, owners[r], d, created_at[k * R + r]) for r in range(R)]
        solved = [(c, r, b) for r, (b, c) in enumerate(mine_batch(tmpls, d, start, count)) if b is not None]
        if not solved:
            break
        c, r, b = min(solved, key=lambda e: e[:2])
        blocks.insert(0, b)
        winners.insert(0, r)
        counters.insert(0, c)
        last = b
    return blocks, winners, counters


@pytest.mark.parametrize("d,owners,start,count", [
    (6, [0, 1, 2], 0, 1 << 12),
    (5, [5, 261, 9, 9], 62 ** 2 - 20, 1 << 10),  # ties among equal low bytes
    (0, [3, 4], 62 ** 4 - 3, 5),                 # every counter solves: position 0 at ctr_start
    (9, [1, 2], 0, 100),                         # stops early at some height
])
def test_statement_is_the_composition(d, owners, start, count):
    parent = ru.genesis()
    n, R = 4, len(owners)
    created = ru.times(n, R) if 9 not in owners else [1_700_000_000 + k for k in range(n) for _ in range(R)]
    got = mine_race(parent, n, d, owners, created, start, count)
    want = by_composition(parent, n, d, owners, created, start, count)
    assert got[1:] == want[1:] and ru.raw(got[0]) == ru.raw(want[0])
    if d == 0:
        assert got[1] == [0] * n and got[2] == [start] * n
    if d == 9:
        assert len(got[0]) < n
    if d == 5:
        assert all(w in (0, 2) for w in got[1])  # 261 never beats 5, the second 9 never the first


def test_one_rival_is_the_chain_statement():
    parent = ru.genesis()
    created = [1_700_000_000 + 3 * k for k in range(3)]
    blocks, winners, counters = mine_race(parent, 3, 6, [4], created, 0, 1 << 12)
    assert ru.raw(blocks) == ru.raw(mine_chain(parent, 3, 6, 4, created, 0, 1 << 12)) and winners == [0, 0, 0]
    assert [field(b, "nonce") for b in blocks] == [nonce_from_counter(c) for c in counters]
    assert mine_race(parent, 0, 6, [1, 2]) == ([], [], [])
    for bad in (dict(difficulty=257), dict(owners=[]), dict(owners=[0] * 257), dict(ctr_start=62 ** 9 - 1, ctr_count=2),
                dict(created_at=[1, 2, 3])):
        a = dict(parent=parent, n=2, difficulty=6, owners=[1, 2], created_at=None, ctr_start=0, ctr_count=16)
        a.update(bad)
        with pytest.raises(ValueError):
            mine_race(**a)


# ---- argument errors of the C entry point: no GPU behind any of them ----
LIMIT = 62 ** 9
BIG = (1 << 24) + 1


@pytest.mark.parametrize("kw,text", [
    (dict(), "null"),                                         # a null ctx
    (dict(parent=None), "null"),
    (dict(out=None), "null"),
    (dict(owners=None), "null"),
    (dict(difficulty=257), "257"),
    (dict(ctr_count=0), "ctr_count"),
    (dict(ctr_count=(1 << 32) + 1), "ctr_count"),
    (dict(ctr_start=LIMIT - 10, ctr_count=11), "62^9"),
    (dict(ctr_start=LIMIT, ctr_count=1), "62^9"),
    (dict(n=BIG), "too large"),
    (dict(n_rivals=0), "n_rivals"),
    (dict(n_rivals=257), "n_rivals"),
    # the order of the checks: each earlier one wins
    (dict(difficulty=257, ctr_count=0, ctr_start=LIMIT, n=BIG, n_rivals=0, parent=None), "257"),
    (dict(ctr_count=0, ctr_start=LIMIT, n=BIG, n_rivals=0, parent=None), "ctr_count"),
    (dict(ctr_start=LIMIT, n=BIG, n_rivals=0, parent=None), "62^9"),
    (dict(n=BIG, n_rivals=0, parent=None), "too large"),
    (dict(n_rivals=257, parent=None, out=None, owners=None), "n_rivals"),
])
def test_error_returns_without_a_gpu(kw, text):
    L = _lib.load()
    a = dict(parent=ctypes.pointer(make_block(1, 0, 9, 1_700_000_000)), n=1, difficulty=4, owners=(ctypes.c_uint32 * 2)(1, 2),
             n_rivals=2, ctr_start=0, ctr_count=1 << 12, out=ctypes.pointer(_lib.Block()))
    a.update(kw)
    mined, hashes = ctypes.c_size_t(7), ctypes.c_uint64(8)
    win, ctr = ctypes.c_uint32(9), ctypes.c_uint64(10)
    before = bytes(a["out"].contents) if a["out"] is not None else None
    rc = L.pow_mine_race(None, a["parent"], a["n"], a["difficulty"], a["owners"], a["n_rivals"], None, a["ctr_start"],
                         a["ctr_count"], None, 0, a["out"], ctypes.byref(win), ctypes.byref(ctr), ctypes.byref(mined),
                         ctypes.byref(hashes))
    assert rc == _lib.POW_EINVAL
    assert text in (L.pow_last_error() or b"").decode()
    assert (mined.value, hashes.value, win.value, ctr.value) == (7, 8, 9, 10)  # nothing is written on an argument error
    if before is not None:
        assert bytes(a["out"].contents) == before


def test_empty_race_still_needs_a_context():
    L = _lib.load()
    assert L.pow_mine_race(None, None, 0, 4, None, 2, None, 0, 1, None, 0, None, None, None, None, None) == _lib.POW_EINVAL
    assert "null" in (L.pow_last_error() or b"").decode()
    assert "pow_mine_race" in _lib.EXPORTS


def test_plan_under_sanitizers(tmp_path):
    """tests/race_plan_unit.cpp links pow_host.cpp alone and runs as a process
    of its own: nothing is loaded into Python."""
    exe = str(tmp_path / "race_plan_unit")
    # no ROCm include path: pow_host.cpp and its headers are HIP-free
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "race_plan_unit.cpp"), os.path.join(CSRC, "pow_host.cpp"), "-o", exe],
                   check=True, cwd=str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert " plans, 0 failed" in r.stdout, r.stdout
