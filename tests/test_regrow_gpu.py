"""One context through calls of growing and shrinking sizes: the buffers of
pow_hash_blocks, pow_verify_chain, pow_verify_chains and pow_sweep are made at
the first call that needs them and grow with a later call's size (the holders
of csrc/pow_ctx.h), and the two verify calls share a tile.  The other suites
mostly open a context per shape.  Every expected value is hashlib's or the
host mirror's."""
import hashlib

import pytest

from mpi_blockchain_amd.miner import GpuMiner

import helpers
import seam_util as su
import verify_chains_util as cu
import verify_util as vu

pytestmark = pytest.mark.gpu

D = cu.D
SWEEP_D, SWEEP_COUNT = 11, 1 << 14  # hashlib finds 10 solutions of template S0 there


def check_chain(m, chain):
    want = vu.mirror(chain, D)
    r = m.verify_chain(chain, D)
    bad = [i for i, s in enumerate(want) if s]
    assert r.status.tolist() == want
    assert (r.ok, r.first_bad, r.n_bad) == (not bad, bad[0] if bad else len(chain), len(bad))
    assert m.stats()["hashes"] == len(chain)


def test_one_context_through_growing_and_shrinking_calls(templates):
    chain = vu.build_chain(9, D, seed=11)
    broken = vu.copy_chain(chain)
    vu.break_prev(broken, 4)
    assert any(vu.mirror(broken, D)) and not any(vu.mirror(chain, D))
    with GpuMiner(0) as m:
        # 1. pow_hash_blocks: the message and digest buffers grow at 5 and serve 3 as they are
        for n in (2, 5, 3):
            blocks = [chain[i] for i in range(n)]
            assert m.hash_blocks(blocks) == [hashlib.sha256(vu.message(b)).hexdigest() for b in blocks]
            assert m.stats()["hashes"] == n
        # 2. pow_verify_chain: the tile grows at 9; the 9 blocks hold the broken link
        check_chain(m, vu.copy_chain(chain, 6, 9))
        check_chain(m, broken)
        check_chain(m, vu.copy_chain(chain, 0, 2))
        # 3. pow_verify_chains: 2, 5, then 1 chains of 2 to 4 blocks (the offsets and
        # verdicts grow at 5, the tile at 5 chains' 15 blocks), one of them with a
        # broken link; then pow_verify_chain again through the tile they share
        for lengths in ((2, 4), (3, 2, 4, 2, 4), (3,)):
            chains = cu.neighbours(len(lengths), 4)
            chains = [vu.copy_chain(c, 0, n) for c, n in zip(chains, lengths)]
            if len(chains) == 5:
                vu.break_prev(chains[2], 1)
            status, first, n_bad, best, ok = cu.expected(chains, D)
            assert ok == (len(chains) != 5)
            r = m.verify_chains(chains, D)
            assert [st.tolist() for st in r.status] == [list(st) for st in status]
            assert (r.first_bad, r.n_bad, r.best, r.ok) == (first, n_bad, best, ok)
            assert m.stats()["hashes"] == sum(lengths)
        check_chain(m, broken)
        # 4. pow_sweep: the list, its twin and the sort's scratch at 16, 64, then 16 entries
        t = templates["S0"]
        want = su.want_list(t, 0, SWEEP_COUNT, SWEEP_D)
        assert 1 <= len(want) <= 16
        tmpl = helpers.block_from_template(t)
        for cap in (16, 64, 16):
            assert m.sweep(tmpl, 0, SWEEP_COUNT, SWEEP_D, cap=cap).tolist() == want
