"""pow_mine_chain on the host (CPU only): its statement
mpi_blockchain_amd.block.mine_chain against a chain mined through the
reference's own block_to_hash and solves_problem
(tests/golden/mined_chain.json), the argument errors of the C entry point,
which need no GPU, and the pure plans of its and pow_mine_batch's fused paths
(csrc/pow_host.cpp) under sanitizers in a process of their own."""
import ctypes
import os
import subprocess

import pytest

from mpi_blockchain_amd import _lib
from mpi_blockchain_amd.block import field, make_block, mine_chain, nonce_from_counter, set_field, verify_chain

import chain_util as cu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpi_blockchain_amd", "csrc")


@pytest.fixture(scope="module")
def recorded():
    return cu.fixture()


@pytest.fixture(scope="module")
def stated(recorded):
    v, parent, _ = recorded
    return mine_chain(parent, len(v["chain"]), v["difficulty"], v["owner"], v["created_at"], v["ctr_start"], 1 << 16)


def test_statement_gives_the_recorded_chain(recorded, stated):
    v, parent, want = recorded
    assert len(want) == 6 and v["difficulty"] == 8
    assert cu.raw(stated) == cu.raw(want)
    # the recorded counters are the lowest from 0: they are the nonces
    for b, ctr in zip(stated, v["counters"]):
        assert field(b, "nonce") == nonce_from_counter(ctr)
    assert any(c > 0 for c in v["counters"])
    assert stated[-1].index == parent.index + 1 and stated[0].index == parent.index + 6
    assert sum(b.created_at > 1 << 32 for b in stated) == 1


def test_statement_passes_the_audit(recorded, stated):
    v, parent, _ = recorded
    assert verify_chain(stated, v["difficulty"]) == [0] * 6
    # ... and links to the parent it was mined on
    assert verify_chain(list(stated) + [parent], 0)[:6] == [0] * 6


def test_statement_is_tip_first_and_stops_at_an_empty_window(recorded, stated):
    v, parent, _ = recorded
    ctrs = list(reversed(v["counters"]))  # mining order
    k = next(i for i, c in enumerate(ctrs) if c == max(ctrs))
    short = mine_chain(parent, 6, v["difficulty"], v["owner"], v["created_at"], 0, max(ctrs))  # excludes that counter
    assert len(short) == k
    assert cu.raw(short) == cu.raw(stated[6 - k:])
    assert mine_chain(parent, 0, 8) == []
    with pytest.raises(ValueError):
        mine_chain(parent, 1, 257)


def test_statement_copies_the_parent_whole():
    """Padding bytes, the bytes of block_hash behind the text and a parent
    hash without a NUL all travel down the chain (node.cpp:292-299, 318)."""
    parent = make_block(254, 9, 3, 5, nonce=b"x" * 10)
    ctypes.memset(ctypes.addressof(parent) + 12, 0xEE, 4)
    ctypes.memset(ctypes.addressof(parent) + 546, 0xDD, 6)
    junk = bytes(1 + i % 255 for i in range(256))
    set_field(parent, "block_hash", junk)
    c = mine_chain(parent, 3, 4, 0x1FF, [1 << 33, 7, 8], 0, 1 << 12)
    assert len(c) == 3 and [b.index for b in c] == [257, 256, 255]
    first = c[2]
    assert field(first, "previous_block_hash") == junk
    assert field(first, "block_hash")[65:] == junk[65:] and field(first, "block_hash")[64] == 0
    for b in c:
        r = cu.raw([b])
        assert r[12:16] == b"\xEE" * 4 and r[546:] == b"\xDD" * 6
        assert b.node_owner_number == 0x1FF and b.difficulty == 4
    assert field(c[0], "previous_block_hash") == field(c[1], "block_hash")
    assert field(c[0], "block_hash")[65:] == junk[65:]


# ---- argument errors of the C entry point: no GPU behind any of them ----
LIMIT = 62 ** 9


@pytest.mark.parametrize("kw,text", [
    (dict(), "null"),                                         # a null ctx
    (dict(parent=None), "null"),
    (dict(out=None), "null"),
    (dict(difficulty=257), "257"),
    (dict(ctr_count=0), "ctr_count"),
    (dict(ctr_count=(1 << 32) + 1), "ctr_count"),
    (dict(ctr_start=LIMIT - 10, ctr_count=11), "62^9"),
    (dict(ctr_start=LIMIT, ctr_count=1), "62^9"),
    (dict(n=(1 << 24) + 1), "too large"),
])
def test_error_returns_without_a_gpu(kw, text):
    L = _lib.load()
    a = dict(parent=ctypes.pointer(cu.genesis()), n=1, difficulty=4, ctr_start=0, ctr_count=1 << 12,
             out=ctypes.pointer(_lib.Block()))
    a.update(kw)
    mined = ctypes.c_size_t(7)
    rc = L.pow_mine_chain(None, a["parent"], a["n"], a["difficulty"], 0, None, a["ctr_start"], a["ctr_count"], None, 0,
                          a["out"], ctypes.byref(mined), None)
    assert rc == _lib.POW_EINVAL
    assert text in (L.pow_last_error() or b"").decode()
    assert mined.value == 7  # nothing is written on an argument error


def test_empty_chain_still_needs_a_context():
    L = _lib.load()
    assert L.pow_mine_chain(None, None, 0, 4, 0, None, 0, 1, None, 0, None, None, None) == _lib.POW_EINVAL
    assert "pow_mine_chain" in _lib.EXPORTS


def test_plans_under_sanitizers(tmp_path):
    """tests/fused_plan_unit.cpp links pow_host.cpp alone and runs as a process
    of its own: nothing is loaded into Python."""
    exe = str(tmp_path / "fused_plan_unit")
    # no ROCm include path: pow_host.cpp and its headers are HIP-free
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "fused_plan_unit.cpp"), os.path.join(CSRC, "pow_host.cpp"), "-o", exe],
                   check=True, cwd=str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert " plans, 0 failed" in r.stdout, r.stdout
