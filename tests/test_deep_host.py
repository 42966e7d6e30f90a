"""The certified deep stretch of tests/golden/deep_stretch.json on the CPU:
every recorded row against hashlib, the stretch's shape, two slices swept again
with the C oracle, and the host statements of pow_mine_chain, pow_mine_batch
and pow_mine_race around its solution, whose sealed bytes are what the GPU
tests (test_deep_gpu.py) expect.  Nothing here runs the code under test, and
no row is left out."""
import ctypes

import numpy as np
import pytest

from oracle.oracle import OBlock, Oracle, make_oblock, py_nonce_from_counter

import deep_util as du

OFFSET = 300_000_007  # where the second slice starts, from empty_from: inside any stretch (NEED > 9 * 10^8)


def test_every_row_is_hashlibs():
    s = du.stretch()
    rows = s["rows"]
    assert 0 < len(rows) <= 1000 and rows == sorted(rows) and len({c for c, _ in rows}) == len(rows)
    assert all(s["empty_from"] <= c <= s["counter"] and z >= s["threshold"] == 24 for c, z in rows)
    for c, z in rows:
        assert du.lz_of(du.digest_of(c)) == z, c
    # about one hit per 2^24 counters: a sweep that lost most of its hits would show here
    n = s["counter"] - s["empty_from"]
    assert n / 2 ** 24 / 2 <= len(rows) <= 2 * n / 2 ** 24 + 10


def test_the_stretch_is_empty_and_long_enough():
    s = du.stretch()
    a, b = s["empty_from"], s["counter"]
    assert s["difficulty"] == 30 and s["owner"] == du.OWNERS[0]
    assert [c for c, z in s["rows"] if z >= 30] == [b]
    assert b - a >= du.NEED and b - a <= 2 ** 32 - 1 and a >= 0 and a > s["previous_solution"]
    assert du.digest_of(b).hex() == s["digest"] and du.lz_of(du.digest_of(b)) == s["leading_zeros"] >= 30
    # the owners of the batch and of the race hash the same message
    assert du.OWNERS[0] & 255 == du.OWNERS[1] & 255 and du.OWNERS[0] != du.OWNERS[1]
    for start, count, solves in du.rows().values():
        assert (start <= b < start + count) == solves and a <= start


@pytest.mark.parametrize("which", ["end", "inside"])
def test_oracle_sweeps_the_slices_again(which):
    s = du.stretch()
    a, b = s["empty_from"], s["counter"]
    lo = b + 1 - du.SLICE if which == "end" else a + OFFSET
    assert a <= lo and lo + du.SLICE <= b + 1
    L = Oracle().L
    L.oracle_sweep_lz.argtypes = [ctypes.POINTER(OBlock), ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint,
                                  ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint8),
                                  ctypes.c_size_t, ctypes.c_int]
    L.oracle_sweep_lz.restype = ctypes.c_size_t
    tmpl = make_oblock(s["parent"]["index"] + 1, s["owner"], s["difficulty"], s["created_at"], bytes(256))
    cap = 4096
    ctr, lz = np.zeros(cap, np.uint32), np.zeros(cap, np.uint8)
    n = L.oracle_sweep_lz(ctypes.byref(tmpl), lo, du.SLICE, s["threshold"],
                          ctr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                          lz.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), cap, 4)
    assert n <= cap
    got = [[lo + int(c), int(z)] for c, z in zip(ctr[:n], lz[:n])]
    assert got == [r for r in s["rows"] if lo <= r[0] < lo + du.SLICE]
    if which == "end":
        assert got[-1] == [b, s["leading_zeros"]]


def test_statements_seal_the_solution():
    """block.mine_chain, block.mine_batch and block.mine_race over the 100
    counters around the solution return it, and their blocks are the template
    sealed by hashlib: the nonce of the counter, the digest's hex and a NUL."""
    s = du.stretch()
    b = s["counter"]
    assert du.stated_chain() == du.sealed(5)
    assert du.stated_chain()[24:34] == py_nonce_from_counter(b)
    assert du.stated_batch() == (du.sealed(5) + du.sealed(261), [b, b])
    assert du.stated_race((5, 261)) == (du.sealed(5), [0], [b])   # a tie: position 0 wins
    assert du.stated_race((261, 5)) == (du.sealed(261), [0], [b])
    assert du.stated_race((5,)) == (du.sealed(5), [0], [b])
    assert du.sealed(5) != du.sealed(261) and du.sealed(5)[:4] + du.sealed(5)[8:] == du.sealed(261)[:4] + du.sealed(261)[8:]
