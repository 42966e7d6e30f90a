"""pow_mine_batch on the host (CPU only): its statement
mpi_blockchain_amd.block.mine_batch against templates mined through the
reference's own block_to_hash and solves_problem
(tests/golden/mined_batch.json), and the argument errors of the C entry point,
which need no GPU."""
import ctypes

import pytest

from mpi_blockchain_amd import _lib
from mpi_blockchain_amd.block import field, make_block, mine_batch, nonce_from_counter, set_field, verify_chain

import batch_util as bu


@pytest.fixture(scope="module")
def recorded():
    return bu.fixture()


@pytest.fixture(scope="module")
def stated(recorded):
    v, tmpls, _ = recorded
    return mine_batch(tmpls, v["difficulty"], v["ctr_start"], 1 << 16)


def test_statement_gives_the_recorded_batch(recorded, stated):
    v, tmpls, sealed = recorded
    assert len(sealed) == 6 and v["difficulty"] == 8
    assert [c for _, c in stated] == v["counters"]
    assert bu.raw([b for b, _ in stated]) == bu.raw(sealed)
    for (b, ctr), t in zip(stated, tmpls):
        assert field(b, "nonce") == nonce_from_counter(ctr)  # the library's own counter map agrees
        assert verify_chain([b], v["difficulty"]) == [0]
    assert any(c > 0 for c in v["counters"])
    # the traps the fixture carries
    assert sum(t.created_at > 1 << 32 for t in tmpls) == 1
    assert sum(t.index >= 256 for t in tmpls) == 1
    tails = [field(t, "previous_block_hash") for t in tmpls]
    assert sum(p[64] == 0 and 0 not in p[65:] for p in tails) == 1


def test_an_unsolved_window_leaves_the_others_alone(recorded, stated):
    v, tmpls, _ = recorded
    top = max(v["counters"])
    short = mine_batch(tmpls, v["difficulty"], 0, top)  # excludes that counter
    for (b, c), (sb, sc), ctr in zip(stated, short, v["counters"]):
        if ctr == top:
            assert (sb, sc) == (None, None)
        else:
            assert sc == c and bu.raw([sb]) == bu.raw([b])
    assert sum(b is None for b, _ in short) == 1
    assert mine_batch([], 8) == []
    with pytest.raises(ValueError):
        mine_batch(tmpls, 257)
    with pytest.raises(ValueError):
        mine_batch(tmpls, 8, 62 ** 9 - 1, 2)


def test_statement_copies_the_template_whole():
    """Padding bytes, the bytes of block_hash behind the text and a previous
    hash without a NUL are kept (node.cpp:318); the template's own nonce is not."""
    t = make_block(254, 0x1FF, 3, (1 << 33) + 5, prev=bytes(1 + i % 255 for i in range(256)), nonce=b"x" * 10)
    ctypes.memset(ctypes.addressof(t) + 12, 0xEE, 4)
    ctypes.memset(ctypes.addressof(t) + 546, 0xDD, 6)
    junk = bytes(255 - i % 255 for i in range(256))
    set_field(t, "block_hash", junk)
    before = bu.raw([t])
    (b, ctr), = mine_batch([t], 4, 0, 1 << 12)
    assert bu.raw([t]) == before  # the template is only read
    r = bu.raw([b])
    assert r[:24] == before[:24] and r[34:290] == before[34:290]  # header, padding and previous hash
    assert r[12:16] == b"\xEE" * 4 and r[546:] == b"\xDD" * 6
    assert r[24:34] == nonce_from_counter(ctr)
    assert r[290 + 64] == 0 and r[290 + 65:546] == junk[65:]
    assert verify_chain([b], 4) == [0]
    # d = 0: every counter solves, the lowest is ctr_start itself
    (_, c0), = mine_batch([t], 0, 62 ** 4 - 3, 5)
    assert c0 == 62 ** 4 - 3


# ---- argument errors of the C entry point: no GPU behind any of them ----
LIMIT = 62 ** 9


@pytest.mark.parametrize("kw,text", [
    (dict(), "null"),                                         # a null ctx
    (dict(tmpls=None), "null"),
    (dict(out=None), "null"),
    (dict(difficulty=257), "257"),
    (dict(ctr_count=0), "ctr_count"),
    (dict(ctr_count=(1 << 32) + 1), "ctr_count"),
    (dict(ctr_start=LIMIT - 10, ctr_count=11), "62^9"),
    (dict(ctr_start=LIMIT, ctr_count=1), "62^9"),
    (dict(n=(1 << 24) + 1), "too large"),
    # the order of the checks: each earlier one wins
    (dict(difficulty=257, ctr_count=0, n=(1 << 24) + 1), "257"),
    (dict(ctr_count=0, ctr_start=LIMIT, n=(1 << 24) + 1), "ctr_count"),
    (dict(ctr_start=LIMIT, n=(1 << 24) + 1), "62^9"),
    (dict(n=(1 << 24) + 1, tmpls=None), "too large"),
])
def test_error_returns_without_a_gpu(kw, text):
    L = _lib.load()
    a = dict(tmpls=ctypes.pointer(make_block(1, 0, 9, 1_700_000_000)), n=1, difficulty=4, ctr_start=0,
             ctr_count=1 << 12, out=ctypes.pointer(_lib.Block()))
    a.update(kw)
    solved, hashes, ctr = ctypes.c_size_t(7), ctypes.c_uint64(8), ctypes.c_uint64(9)
    before = bytes(a["out"].contents) if a["out"] is not None else None
    rc = L.pow_mine_batch(None, a["tmpls"], a["n"], a["difficulty"], a["ctr_start"], a["ctr_count"], None, 0, a["out"],
                          ctypes.byref(ctr), ctypes.byref(solved), ctypes.byref(hashes))
    assert rc == _lib.POW_EINVAL
    assert text in (L.pow_last_error() or b"").decode()
    assert (solved.value, hashes.value, ctr.value) == (7, 8, 9)  # nothing is written on an argument error
    if before is not None:
        assert bytes(a["out"].contents) == before


def test_empty_batch_still_needs_a_context():
    L = _lib.load()
    assert L.pow_mine_batch(None, None, 0, 4, 0, 1, None, 0, None, None, None, None) == _lib.POW_EINVAL
    assert "null" in (L.pow_last_error() or b"").decode()
    assert "pow_mine_batch" in _lib.EXPORTS
