"""pow_verify_chains on the host (CPU only): its statements
mpi_blockchain_amd.block.verify_chains and best_chain on the layouts the GPU
tests use, and the argument errors of the C entry point, which need no GPU."""
import ctypes

import pytest

from mpi_blockchain_amd import _lib
from mpi_blockchain_amd.block import V_HASH, V_LINK, best_chain, make_block, verify_chain, verify_chains

import verify_chains_util as cu
import verify_util as vu

D = cu.D


@pytest.fixture(scope="module")
def chain200():
    return vu.build_chain(200, D, seed=5)


@pytest.mark.parametrize("lengths", cu.SPLITS, ids=lambda s: f"{len(s)}pieces")
def test_pieces_of_a_valid_chain_are_valid(chain200, lengths):
    pieces = cu.split(chain200, lengths)
    got = verify_chains(pieces, D)
    assert got == [verify_chain(p, D) for p in pieces]
    assert [len(g) for g in got] == list(lengths) and not any(any(g) for g in got)


def test_unrelated_neighbours_do_not_link():
    chains = cu.neighbours()
    assert verify_chains(chains, D) == [[0] * 5] * 13
    arr, total = cu.concat(chains)
    one = verify_chain(arr, D)  # the same buffer as one chain: every boundary is a broken link
    assert total == 65 and all(one[5 * c + 4] for c in range(12)) and not one[64]


def test_a_boundary_cuts_the_link(chain200):
    lengths = cu.SPLITS[2]
    for k in range(len(lengths) - 1):
        whole = vu.copy_chain(chain200)
        tip = sum(lengths[:k + 1])
        vu.flip_hash_digit(whole, tip)
        got = verify_chains(cu.split(whole, lengths), D)
        assert [(c, i, s) for c, st in enumerate(got) for i, s in enumerate(st) if s] == [(k + 1, 0, V_HASH)]
        assert verify_chain(whole, D)[tip - 1] == V_LINK  # as one chain the block in front of it links to it


def tips(*indices):
    return [[make_block(i)] for i in indices]


def test_best_chain():
    clean = lambda chains: [[0] * len(c) for c in chains]  # noqa: E731
    c = tips(7, 9, 8)
    assert best_chain(c, clean(c)) == 1                      # the highest tip index wins
    c = tips(9, 3, 9, 9)
    assert best_chain(c, clean(c)) == 0                      # a tie goes to the lowest position
    c = tips(5, 9, 8)
    assert best_chain(c, [[0], [V_HASH], [0]]) == 2          # a flagged chain with the highest tip is skipped
    c = [[make_block(4), make_block(900)], [make_block(6), make_block(5)]]
    assert best_chain(c, clean(c)) == 1                      # the tip is the first block, not the highest index inside
    assert best_chain(c, [[0, 0], [0, V_LINK]]) == 0         # a flag anywhere in the chain disqualifies it
    c = [[], [make_block(2)], []]
    assert best_chain(c, clean(c)) == 1                      # empty chains never win
    assert best_chain([[], []], [[], []]) is None
    assert best_chain([], []) is None
    c = tips(3, 4)
    assert best_chain(c, [[V_HASH], [V_LINK]]) is None       # none valid
    c = tips(0, 0xFFFFFFFF, 0x80000000)
    assert best_chain(c, clean(c)) == 1                      # plain unsigned: 0xFFFFFFFF is the greatest, not -1
    c = tips(0, 0)
    assert best_chain(c, clean(c)) == 0


# ---- argument errors of the C entry point: no GPU behind any of them ----
MAXC = 1 << 20
FAKE_CTX = ctypes.create_string_buffer(1 << 16)  # non-null, never reached: the checks come before the context is touched


def u32(*v):
    return (ctypes.c_uint32 * len(v))(*v)


@pytest.mark.parametrize("kw,text", [
    (dict(), "null"),                                              # a null ctx
    (dict(ctx=FAKE_CTX, lengths=None), "null"),
    (dict(ctx=FAKE_CTX, blocks=None), "null"),
    (dict(n_chains=0, lengths=None, blocks=None), "null"),         # an empty batch still needs a context
    (dict(lengths=u32(1 << 24)), "null"),                          # 2^24 blocks are allowed: the null ctx is what fails
    (dict(difficulty=257), "257"),
    (dict(n_chains=MAXC + 1, lengths=u32(*([0] * (MAXC + 1)))), "too many"),
    (dict(lengths=u32((1 << 24) + 1)), "too large"),
    (dict(n_chains=3, lengths=u32(1 << 23, 1 << 23, 1)), "too large"),
    (dict(n_chains=2, lengths=u32(0xFFFFFFFF, 0xFFFFFFFF)), "too large"),  # no 32-bit wrap of the sum
    # the order of the checks: each earlier one wins
    (dict(difficulty=257, n_chains=MAXC + 1, lengths=None, blocks=None), "257"),
    (dict(n_chains=MAXC + 1, lengths=u32(*([1 << 24] * (MAXC + 1))), blocks=None), "too many"),
    (dict(ctx=FAKE_CTX, lengths=u32((1 << 24) + 1), blocks=None), "too large"),
])
def test_error_returns_without_a_gpu(kw, text):
    L = _lib.load()
    a = dict(ctx=None, blocks=ctypes.pointer(make_block(1, 0, 9, 1_700_000_000)), lengths=u32(1), n_chains=1,
             difficulty=4)
    a.update(kw)
    status = (ctypes.c_uint8 * 4)(*[0xAB] * 4)
    first, bad, best = u32(7, 7), u32(8, 8), ctypes.c_size_t(9)
    rc = L.pow_verify_chains(a["ctx"], a["blocks"], a["lengths"], a["n_chains"], a["difficulty"], status, first, bad,
                             ctypes.byref(best))
    assert rc == _lib.POW_EINVAL
    assert text in (L.pow_last_error() or b"").decode()
    # nothing is written on an argument error
    assert (list(status), list(first), list(bad), best.value) == ([0xAB] * 4, [7, 7], [8, 8], 9)


def test_entry_point_is_exported():
    assert "pow_verify_chains" in _lib.EXPORTS
    assert hasattr(_lib.load(), "pow_verify_chains") and hasattr(_lib.load(test_hooks=True), "pow_verify_chains")
