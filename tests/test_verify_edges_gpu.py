"""pow_verify_chain's C-string link compare and hex compare on the GPU, at
their edges.  The kernel compares dwords that sit two bytes off the fields,
masks the first and the last one, finds the first NUL with a bit trick and
builds the digest's hex text arithmetically: the chains of tests/verify_edges.py
put a NUL in every byte lane and at both ends of the field, a difference on
either side of it, and every kind of wrong character at every text position.

The expected status is always the mirror's
(mpi_blockchain_amd.block.verify_chain); tests/test_verify_edges_host.py
asserts on the CPU that the chains hold the outcomes they are meant to."""
import random

import numpy as np
import pytest

from mpi_blockchain_amd.block import V_HASH, V_LINK, field, set_field
from mpi_blockchain_amd.miner import GpuMiner

import verify_edges as ve
import verify_util as vu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def miner():
    with GpuMiner(0) as m:
        yield m


@pytest.fixture(scope="module")
def hex_chain():
    c = ve.hex_chain()
    base = vu.mirror(c, 0)
    assert not any(base)
    return c, base


def check(miner, chain, want):
    r = miner.verify_chain(chain, 0)
    got = r.status.tolist()
    wrong = [(i, got[i], want[i]) for i in range(len(want)) if got[i] != want[i]]
    assert r.status.dtype == np.uint8 and not wrong, wrong[:10]
    bad = [i for i, s in enumerate(want) if s]
    assert (r.first_bad, r.n_bad, r.ok) == (bad[0] if bad else len(want), len(bad), not bad)
    return r


def test_link_matrix(miner):
    cases = ve.link_cases()
    chain = ve.link_chain(cases)
    want = vu.mirror(chain, 0)
    for k, (pc, pp, kind, a, b) in enumerate(cases):  # the mirror's link flag is the one-line rule
        assert bool(want[2 * k] & V_LINK) == ve.link_differs(a, b), (pc, pp, kind)
    r = check(miner, chain, want)
    got = r.status.tolist()
    for k, (pc, pp, kind, a, b) in enumerate(cases):
        assert bool(got[2 * k] & V_LINK) == ve.link_differs(a, b), (pc, pp, kind)
    assert miner.stats()["launches"] == 1


def test_hex_matrix_clean(miner, hex_chain):
    c, base = hex_chain
    check(miner, c, base)


@pytest.mark.parametrize("kind", ve.HEX_KINDS)
def test_hex_matrix(miner, hex_chain, kind):
    c, base = hex_chain
    bad, used = ve.corrupt_hex(c, kind)
    want = vu.expected_after(base, bad, list(used), 0)
    for i in used:
        assert want[i] == V_HASH  # that and nothing else on the block itself
    r = check(miner, bad, want)
    assert [i for i, s in enumerate(r.status.tolist()) if s & V_HASH] == sorted(used)


def test_hash_terminator_and_the_bytes_behind_it(miner, hex_chain):
    c, base = hex_chain
    # block_hash[64] is the text's NUL: any other byte there flags the block
    bad = vu.copy_chain(c)
    touched = {0: 1, 31: 0x80, 96: 0xFF, 63: ord("0")}
    for i, v in touched.items():
        ve.set_hash_byte(bad, i, 64, v)
    want = vu.expected_after(base, bad, list(touched), 0)
    assert all(want[i] == V_HASH for i in touched)
    check(miner, bad, want)
    # block_hash[65..255] is behind it: no check reads it (the children's links are C strings too)
    rng = random.Random(11)
    junk = vu.copy_chain(c)
    for i in range(len(junk)):
        raw = field(junk[i], "block_hash")
        tail = bytes(rng.randrange(256) for _ in range(191))
        if i in (0, 31, 63, 96):
            tail = bytes([0xFF, 0x80, 1]) + tail[3:]  # right behind the NUL
        set_field(junk[i], "block_hash", raw[:65] + tail)
    assert vu.mirror(junk, 0) == base
    check(miner, junk, base)
