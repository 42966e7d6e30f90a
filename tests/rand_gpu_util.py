"""What the GPU tests of pow_mine_rand (K8) share: contexts of the test library
under its three switches, the call through the C ABI with poisoned outputs, and
the brute force of tests/rand_util.py, computed once per case."""
import ctypes
import functools

import helpers
import rand_util
from mpi_blockchain_amd import _lib

SWITCHES = ("POW_RAND_RUN", "POW_RAND_LANES_LOG2", "POW_RAND_LAUNCH_LOG2")
SEED = 1700000003  # time + rank
POISON = b"\xA5" * 552


def miner_with(**switches):
    """A context of the test library whose pow_init saw the given switches."""
    return helpers.hooked_miner(SWITCHES, **switches)


def raw(b) -> bytes:
    return ctypes.string_at(ctypes.addressof(b), ctypes.sizeof(b))


def block_of(data: bytes) -> _lib.Block:
    b = _lib.Block()
    ctypes.memmove(ctypes.addressof(b), data, len(data))
    return b


@functools.lru_cache(maxsize=None)
def brute(tmpl_bytes: bytes, seed: int, start: int, count: int, d: int, want: int = 1):
    """rand_util's answer, computed once per case and shared."""
    return tuple(rand_util.mine(tmpl_bytes, seed, start, count, d, want))


def call(m, tmpl, seed, start, count, d, cancel=None, epoch=0):
    """pow_mine_rand through the C ABI with poisoned outputs: rc, out's bytes, found, hashes."""
    out = (ctypes.c_char * 552)(*([0xA5] * 552))
    found, hashes = ctypes.c_uint64(12345), ctypes.c_uint64(12345)
    rc = m.L.pow_mine_rand(m.ctx, ctypes.byref(tmpl), seed, start, count, d, cancel, epoch,
                           ctypes.cast(out, ctypes.POINTER(_lib.Block)), ctypes.byref(found), ctypes.byref(hashes))
    return rc, bytes(out), found.value, hashes.value


def check_against(m, tmpl, seed, start, count, d, hit, every_trial=False):
    """One call against `hit`, the lowest solving (trial, nonce, hex digest) of
    the window or None.  every_trial: a window without a solution was hashed
    trial by trial, each exactly once.  Returns the call's hashes."""
    tb = raw(tmpl)
    rc, out, found, hashes = call(m, tmpl, seed, start, count, d)
    if hit is None:
        assert (rc, out, found) == (0, POISON, 12345), (m.L.pow_last_error(), seed, start, count, d)
        assert hashes == count if every_trial else hashes >= count, (hashes, seed, start, count, d)
        return hashes
    trial, nonce, hexd = hit
    assert rc == 1, (m.L.pow_last_error(), seed, start, count, d)
    assert found == trial, (found, trial, seed, start, count, d)
    assert out == rand_util.seal(tb, nonce, hexd)
    assert trial - start + 1 <= hashes <= count, (hashes, trial, start, count)  # up to the answer, none twice
    return hashes


def check_against_brute(m, tmpl, seed, start, count, d):
    """One call against the brute force; the answer's trial, or None."""
    hits = brute(raw(tmpl), seed, start, count, d)
    check_against(m, tmpl, seed, start, count, d, hits[0] if hits else None)
    return hits[0][0] if hits else None
