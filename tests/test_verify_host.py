"""Chain verification on the host (CPU only): the mirror
mpi_blockchain_amd.block.verify_chain, which states what pow_verify_chain
computes on the GPU; the recorded reference chain; and the argument errors of
the C entry point, which need no GPU."""
import ctypes
import hashlib

import pytest

from mpi_blockchain_amd import _lib
from mpi_blockchain_amd.block import V_HASH, V_INDEX, V_LINK, V_WORK, field, make_block, set_field, verify_chain
from oracle.oracle import OBlock, RefLib, ref_available

import verify_util as vu

D = 4


@pytest.fixture(scope="module")
def chain():
    return vu.build_chain(6, D, seed=3)


def test_valid_chain_is_all_zero(chain):
    assert verify_chain(chain, D) == [0] * 6
    assert verify_chain(chain, 0) == [0] * 6
    assert verify_chain([], D) == []
    assert verify_chain(vu.copy_chain(chain, 2, 3), D) == [0]


def test_accepts_a_list_of_blocks(chain):
    assert verify_chain(list(chain), D) == [0] * 6


def with_work(c, want: dict) -> list:
    """`want` (flags by position, V_WORK left out) plus V_WORK wherever the
    block's digest, by hashlib, has fewer than D leading zero bits: a
    corruption that changes the message leaves the work to chance."""
    return [want.get(i, 0) | (V_WORK if vu.leading_zero_bits(c[i]) < D else 0) for i in range(len(c))]


@pytest.mark.parametrize("kind,pos,want", [
    ("nonce", 2, {2: V_HASH}),                        # another digest: the stored text no longer matches
    ("hash_digit", 2, {2: V_HASH, 1: V_LINK}),       # the child links to the stored text
    ("unterminated_hash", 2, {2: V_HASH, 1: V_LINK}),
    ("prev", 2, {2: V_HASH | V_LINK}),                # the link field is part of the message
    ("index", 2, {2: V_HASH | V_INDEX, 1: V_INDEX}),  # so is the index's low byte
    ("prev", 5, {5: V_HASH}),                         # the last block has no parent here: no link check
    ("hash_digit", 0, {0: V_HASH}),                   # the tip has no child
])
def test_each_corruption(chain, kind, pos, want):
    c = vu.copy_chain(chain)
    vu.CORRUPTIONS[kind](c, pos)
    assert verify_chain(c, D) == with_work(c, want)


def test_work_flag_alone(chain):
    z = [vu.leading_zero_bits(b) for b in chain]
    assert min(z) >= D
    got = verify_chain(chain, min(z) + 1)
    assert got == [V_WORK if zi == min(z) else 0 for zi in z] and any(got)
    assert verify_chain(chain, 256) == [V_WORK] * 6
    assert verify_chain(chain, 33) == [V_WORK if zi < 33 else 0 for zi in z]
    with pytest.raises(ValueError):
        verify_chain(chain, 257)


def test_work_is_tested_on_the_computed_digest(chain):
    """A stored text of all zeros buys no work: POW_V_WORK looks at the digest."""
    c = vu.copy_chain(chain)
    set_field(c[0], "block_hash", b"0" * 64)
    z0 = vu.leading_zero_bits(c[0])
    assert verify_chain(c, z0 + 1)[0] == V_HASH | V_WORK
    assert verify_chain(c, z0)[0] == V_HASH


def test_index_wraps_in_uint32(chain):
    c = vu.copy_chain(chain)
    vu.index_wrap(c, 3)  # index 0 over 0xFFFFFFFF: consecutive
    got = verify_chain(c, D)
    assert not got[3] & V_INDEX
    assert got[2] & V_INDEX and got[4] & V_INDEX  # their neighbours no longer are


def test_link_is_a_c_string_compare(chain):
    c = vu.copy_chain(chain)
    # bytes after the parent's NUL do not break the link of its child ...
    raw = bytearray(field(c[3], "block_hash"))
    raw[100:104] = b"junk"
    set_field(c[3], "block_hash", bytes(raw))
    assert verify_chain(c, D) == [0] * 6
    # ... a child that holds only a prefix of the parent's text does
    c = vu.copy_chain(chain)
    raw = bytearray(field(c[2], "previous_block_hash"))
    raw[10] = 0
    set_field(c[2], "previous_block_hash", bytes(raw))
    assert verify_chain(c, D)[2] & V_LINK
    # two fields without any NUL are compared over all 256 bytes
    c = vu.copy_chain(chain)
    full = b"0123456789abcdef" * 16
    set_field(c[2], "previous_block_hash", full)
    set_field(c[3], "block_hash", full)
    assert not verify_chain(c, D)[2] & V_LINK
    set_field(c[3], "block_hash", full[:255] + b"X")
    assert verify_chain(c, D)[2] & V_LINK


def test_combination(chain):
    c = vu.copy_chain(chain)
    vu.flip_hash_digit(c, 1)
    vu.index_off_by_one(c, 3)
    vu.break_prev(c, 4)
    assert verify_chain(c, D) == with_work(c, {0: V_LINK, 1: V_HASH, 2: V_INDEX, 3: V_HASH | V_INDEX,
                                               4: V_HASH | V_LINK})


# ---- the recorded reference chain ----
def test_fixture_chain_passes_the_mirror():
    c, d = vu.fixture_chain()
    assert len(c) == 70 and d == 4
    assert verify_chain(c, d) == [0] * 70
    assert max(b.index for b in c) > 255 and min(b.index for b in c) <= 255
    assert sum(b.created_at > 1 << 32 for b in c) == 1
    tails = [i for i, b in enumerate(c) if field(b, "previous_block_hash").split(b"\0", 1)[1].strip(b"\0")]
    assert len(tails) == 1
    # the bytes after the NUL are hashed: without them the stored hash is wrong
    i = tails[0]
    raw = field(c[i], "previous_block_hash")
    set_field(c[i], "previous_block_hash", raw.split(b"\0", 1)[0])
    assert verify_chain(c, d)[i] & V_HASH and not verify_chain(c, d)[i] & V_LINK


def test_fixture_hashes_are_the_references():
    """Where the reference build exists it still gives the recorded texts;
    everywhere, hashlib over the restated serialisation gives them too."""
    c, _ = vu.fixture_chain()
    R = RefLib("O2") if ref_available() else None
    for b in c:
        stored = field(b, "block_hash").split(b"\0", 1)[0].decode()
        assert hashlib.sha256(vu.message(b)).hexdigest() == stored
        if R:
            ob = OBlock()
            ctypes.memmove(ctypes.addressof(ob), ctypes.addressof(b), ctypes.sizeof(OBlock))
            assert R.block_to_hash(ob) == stored


# ---- argument errors of the C entry point: no GPU behind any of them ----
def _last_error(L) -> str:
    return (L.pow_last_error() or b"").decode()


def test_error_returns_without_a_gpu():
    L = _lib.load()
    b = make_block(1, 0, D, 0)
    first, bad = ctypes.c_size_t(7), ctypes.c_size_t(7)
    assert L.pow_verify_chain(None, ctypes.byref(b), 1, D, None, ctypes.byref(first), ctypes.byref(bad)) == _lib.POW_EINVAL
    assert "null" in _last_error(L)
    assert L.pow_verify_chain(None, ctypes.byref(b), 1, 257, None, None, None) == _lib.POW_EINVAL
    assert "257" in _last_error(L)
    assert L.pow_verify_chain(None, ctypes.byref(b), (1 << 24) + 1, D, None, None, None) == _lib.POW_EINVAL
    assert "too large" in _last_error(L)
    assert L.pow_verify_chain(None, None, 0, 256, None, None, None) == _lib.POW_EINVAL  # n = 0 still needs a ctx
    assert "pow_verify_chain" in _lib.EXPORTS
