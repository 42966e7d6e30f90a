"""The 32-bit difficulty seam on the CPU: the witnesses of
tests/golden/lz_witnesses.json against hashlib, the C oracle's sweep around
them at d = 29..35, and pow_solves_problem at every difficulty 0..256 on the
witnesses' digests and on synthetic ones with a chosen number of leading zero
bits.  The expected values are hashlib's and Python's bit_length."""
import hashlib

import pytest

from mpi_blockchain_amd.block import block_to_str, mine_chain, make_block, solves_problem
from oracle.oracle import Oracle, make_oblock, py_nonce_from_counter

import helpers
import seam_util as su


@pytest.fixture(scope="module")
def O():
    return Oracle()


@pytest.mark.parametrize("name", list(su.SOLVES))
def test_witness_digest_is_hashlibs(templates, name):
    row = next(r for r in su.seam_rows() if r["template"] == name)
    b = helpers.with_nonce(helpers.block_from_template(templates[name]), py_nonce_from_counter(row["counter"]))
    digest = hashlib.sha256(block_to_str(b)).digest()
    assert digest == su.digest_of(templates[name], row["counter"])  # the library's serialisation and Python's
    assert digest.hex() == row["digest"]
    assert su.lz_of(digest) == row["leading_zeros"] == su.SOLVES[name]
    # the digest's first words say which side of the seam it is on
    h0, h1 = int(row["digest"][:8], 16), int(row["digest"][8:16], 16)
    assert {"S2": h0 == 0 and h1 >> 30 == 1, "S1": h0 == 0 and h1 >> 31 == 1, "S0": h0 == 1}[name]


@pytest.mark.parametrize("name", list(su.SOLVES))
def test_oracle_sweep_around_the_witness(O, templates, name):
    t = templates[name]
    row = next(r for r in su.seam_rows() if r["template"] == name)
    start = row["counter"] - su.BEFORE
    ob = make_oblock(t["index"], t["node_owner_number"], t["difficulty"], t["created_at"],
                     bytes.fromhex(t["previous_block_hash_hex"]))
    for d in su.SEAM_D:
        want = su.want_list(t, start, su.WINDOW, d)
        assert want == ([su.BEFORE] if d <= row["leading_zeros"] else []) or d == 29  # the table of the issue
        got, n = O.sweep(ob, start, su.WINDOW, d, threads=2)
        assert (got.tolist(), n) == (want, len(want)), d
        assert O.mine(ob, start, su.WINDOW, d) == (start + want[0] if want else None)
    want4 = su.want_list(t, start, su.WINDOW, 4)
    assert 90 <= len(want4) <= 170  # 2,048 / 16 = 128 expected
    assert O.sweep(ob, start, su.WINDOW, 4, threads=2)[0].tolist() == want4


def test_solves_problem_on_the_witnesses():
    rows = su.seam_rows() + su.witnesses()["chain"]["witnesses"]
    assert len(rows) == 9
    for row in rows:
        lz = 256 - int(row["digest"], 16).bit_length()
        assert lz == row["leading_zeros"]
        for d in range(257):
            assert solves_problem(row["digest"], d) == (d <= lz), (row, d)


def test_solves_problem_on_synthetic_digests():
    cases = su.synthetic_digests()
    assert len(cases) == 513 and {k for k, _ in cases} == set(range(257))
    for k, v in cases:
        assert 256 - v.bit_length() == k
        hexd = f"{v:064x}"
        got = [solves_problem(hexd, d) for d in range(257)]
        assert got == [d <= k for d in range(257)], (k, hexd)


def test_chain_witnesses_are_hashlibs():
    """The pow_mine_chain witnesses (found on the GPU by gen_lz_witnesses.py):
    every recorded digest is hashlib's, a "solves" row has at least d leading
    zero bits and a "misses" row exactly d - 1, alone in a window that the host
    statement finds empty."""
    c = su.witnesses()["chain"]
    p = c["parent"]
    parent = make_block(p["index"], p["node_owner_number"], p["difficulty"], p["created_at"])
    assert (c["before"], c["window"]) == (su.BEFORE, su.WINDOW)
    assert sorted((w["difficulty"], w["kind"]) for w in c["witnesses"]) == \
        sorted((d, k) for d in (31, 32, 33) for k in ("solves", "misses"))
    for w in c["witnesses"]:
        d, ctr = w["difficulty"], w["counter"]
        one = mine_chain(parent, 1, 0, c["owner"], [c["created_at"]], ctr, 1)[0]  # d = 0: counter ctr itself ...
        one.difficulty = d                                                        # ... under the d template's header
        one.nonce = py_nonce_from_counter(ctr)[:9]
        digest = hashlib.sha256(block_to_str(one)).digest()
        assert digest.hex() == w["digest"] and su.lz_of(digest) == w["leading_zeros"]
        got = mine_chain(parent, 1, d, c["owner"], [c["created_at"]], ctr - su.BEFORE, su.WINDOW)
        if w["kind"] == "solves":
            assert w["leading_zeros"] >= d and len(got) == 1
        else:
            assert w["leading_zeros"] == d - 1 and got == []
