"""What the chains of tests/verify_edges.py promise, asserted on the CPU with
the mirror (mpi_blockchain_amd.block.verify_chain): the GPU tests that run
them through pow_verify_chain (tests/test_verify_edges_gpu.py) then cannot
pass on a matrix that misses an outcome."""
import collections

from mpi_blockchain_amd.block import V_HASH, V_LINK, field

import verify_edges as ve
import verify_util as vu


def test_link_matrix_has_both_outcomes_where_both_can():
    cases = ve.link_cases()
    assert 1800 <= len(cases) <= 17 * 17 * 7  # about 2,000: what cannot be built is dropped
    chain = ve.link_chain(cases)
    status = vu.mirror(chain, 0)
    seen = collections.defaultdict(set)
    for k, (pc, pp, kind, a, b) in enumerate(cases):
        assert (field(chain[2 * k], "previous_block_hash"), field(chain[2 * k + 1], "block_hash")) == (a, b)
        differs = ve.link_differs(a, b)
        assert bool(status[2 * k] & V_LINK) == differs, (pc, pp, kind)
        assert status[2 * k] & V_HASH  # nothing was mined: every stored hash is wrong
        seen[(pc, pp)].add(differs)
    assert set(seen) == {(pc, pp) for pc in ve.NUL_AT for pp in ve.NUL_AT}
    for (pc, pp), outcomes in seen.items():
        if pc != pp:
            want = {True}           # C strings of different lengths
        elif pc == 0:
            want = {False}          # two empty strings
        else:
            want = {True, False}    # the one difference in front of the common NUL, or behind it / absent
        assert outcomes == want, (pc, pp, outcomes)
    # the bytes behind the NUL differ in some equal pairs, and the parents' own links mostly fail
    assert any(not ve.link_differs(a, b) and a != b for _, _, _, a, b in cases)
    assert sum(1 for k in range(len(cases)) if status[2 * k + 1] & V_LINK) >= len(cases) - 2


def test_hex_matrix_covers_every_value_at_every_position():
    chain = ve.hex_chain()
    assert not any(vu.mirror(chain, 0))
    texts = [field(b, "block_hash")[:64] for b in chain]
    for p in range(64):
        assert {t[p] for t in texts} == set(b"0123456789abcdef"), p
    for kind in ve.HEX_KINDS:
        bad, used = ve.corrupt_hex(chain, kind)
        assert sorted(used.values()) == list(range(64)) and len(used) == 64
        assert {0, 31, 63, 96} <= set(used)  # lanes 0, 31, 63 of workgroup 0; lane 32 of workgroup 1
        assert not any(i + 1 in used for i in used)
        want = vu.expected_after([0] * len(chain), bad, list(used), 0)
        for i in used:
            assert want[i] == V_HASH, (kind, i, want[i])
        assert all(want[i - 1] in (0, V_LINK) for i in used if i) and sum(1 for s in want if s & V_HASH) == 64
        if kind == "nul":  # a NUL inside the text shortens the parent's C string: the child's link breaks
            assert all(want[i - 1] == V_LINK for i in used if i)
