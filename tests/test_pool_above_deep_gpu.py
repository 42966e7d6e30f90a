"""K14 on the GPU on synthetic forests of up to 2^20 nodes (the pool's limit),
through the test library's pow_test_pool_above: K14a to K14c over 4,096
workgroups and partials, K14d's jumps across levels 12 to 19, its grid of
4,096 x k workgroups, and the drop's keep-marks into K12e and K12f at that
size.  The forests are numpy arrays (tests/pool_deep_util.py) with closed-form
answers or tests/pool_above_util.py's numpy statements; nothing is hashed.
Every comparison is exact."""
import numpy as np
import pytest

from mpi_blockchain_amd._lib import POW_EINVAL
from mpi_blockchain_amd.block import POOL_NONE, POOL_ROOT
from mpi_blockchain_amd.miner import GpuMiner

import pool_above_util as au
import pool_deep_util as du
from pool_above_util import DROP, SUBTREES, TIPS

pytestmark = pytest.mark.gpu

U32 = np.uint32
M = 1 << 20


@pytest.fixture(scope="module")
def gpu():
    with GpuMiner(0, test_hooks=True) as m:
        yield m


@pytest.fixture(scope="module")
def list20():
    """One shuffled list of 2^20 nodes, shared and left unchanged."""
    return du.shuffled_list(M, 20)


def last_error(L) -> str:
    return (L.pow_last_error() or b"").decode()


def above(gpu, F, mode, roots=(), flags=0, fin=0, index=None, n_bad=None):
    n = len(F.parent)
    index = np.arange(n, dtype=U32) % 97 if index is None else index
    n_bad = np.zeros(n, dtype=U32) if n_bad is None else n_bad
    rc, o = au.run_above(gpu.L, gpu.ctx, F.parent, F.depth, index, n_bad, mode, roots, flags, fin)
    assert rc == 0, last_error(gpu.L)
    return o, index, n_bad


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        at = int(np.flatnonzero(got.reshape(-1) != want.reshape(-1))[0])
        raise AssertionError(f"{what}: {int((got != want).sum())} entries differ, the first at {at}: "
                             f"{got.reshape(-1)[at]} for {want.reshape(-1)[at]}")


def check_tips(gpu, F, what, fin=0):
    n = len(F.parent)
    n_bad = (np.arange(n, dtype=U32) % 5 == 0).astype(U32)
    for flags in (0, au.SOUND_ONLY):
        o, _, _ = above(gpu, F, TIPS, flags=flags, fin=fin, n_bad=n_bad)
        marks = au.tips_of(F.parent, n_bad, bool(flags))
        same(o.marks, marks, f"{what}: tip marks")
        assert o.total == int(marks.sum()), (what, o.total)
        same(o.list, np.flatnonzero(marks).astype(U32), f"{what}: the list")


def check_subtrees(gpu, F, roots, want, what, fin=0, index=None, n_bad=None):
    """want: (size, height, key per root, the union's marks)."""
    o, index, n_bad = above(gpu, F, SUBTREES, roots, fin=fin, index=index, n_bad=n_bad)
    size, height, best, on = want(index, n_bad)
    assert o.size.tolist() == list(size), (what, o.size.tolist(), size)
    assert o.height.tolist() == list(height), (what, o.height.tolist(), height)
    assert o.best.tolist() == list(best), (what, [hex(int(x)) for x in o.best], [hex(x) for x in best])
    same(o.marks, on, f"{what}: on")
    assert o.total == int(on.sum()), (what, o.total)


def check_drop(gpu, F, roots, on, what, fin=0):
    o, _, _ = above(gpu, F, DROP, roots, fin=fin)
    keep = (1 - on).astype(np.uint8)
    same(o.marks, keep, f"{what}: keep-marks")
    assert o.total == int(keep.sum()), (what, o.total)
    new, parent, depth = au.dropped(F.parent, F.depth, keep)
    same(o.map, new, f"{what}: map")
    same(o.parent, parent, f"{what}: parent")
    same(o.depth, depth, f"{what}: depth")


def list_answers(L, roots):
    """On one list every node at or over the root's height is a member."""
    def want(index, n_bad):
        size, height, best, on = [], [], [], np.zeros(L.n, dtype=np.uint8)
        for r in roots:
            m = L.depth >= L.depth[r]
            on |= m.astype(np.uint8)
            size.append(int(m.sum())), height.append(L.n - int(L.depth[r])), best.append(au.key_of(index, n_bad, m))
        return size, height, best, on
    return want


# ---- a flat chain of 2^20: every level of the table, 4,096 workgroups a root ----
def test_flat_chain_of_2_20(gpu, list20):
    L = list20
    heights = [1, 2, 3, 1 << 10, (1 << 19) - 1, 1 << 19, (1 << 19) + 1, M - 1, M]
    roots = [int(L.order[h - 1]) for h in heights]
    n_bad = (np.arange(M, dtype=U32) % 3 == 0).astype(U32)
    check_subtrees(gpu, L, roots, list_answers(L, roots), "list of 2^20", n_bad=n_bad)
    o, _, _ = above(gpu, L, SUBTREES, roots)
    assert o.size.tolist() == [M - h + 1 for h in heights] and o.height.tolist() == [M - h for h in heights]
    check_tips(gpu, L, "list of 2^20")
    on = (L.depth >= (1 << 19) + 7).astype(np.uint8)
    check_drop(gpu, L, [int(L.order[(1 << 19) + 6])], on, "list of 2^20, upper half dropped", fin=1)


def test_chains_of_a_power_of_two_and_one_more(gpu):
    for k in (6, 8, 12, 16):
        for n in (1 << k, (1 << k) + 1):
            L = du.shuffled_list(n, k, end=POOL_NONE if k == 8 else POOL_ROOT)
            roots = [int(L.order[0]), int(L.order[1]), int(L.order[n // 2]), int(L.order[n - 1])]
            check_subtrees(gpu, L, roots, list_answers(L, roots), f"list of {n}")
            check_drop(gpu, L, roots[2:], (L.depth >= n // 2 + 1).astype(np.uint8), f"list of {n}")
            check_tips(gpu, L, f"list of {n}")


# ---- a star of 2^20: every node but one a tip, 4,096 partials ----
def test_star_of_2_20(gpu):
    perm = np.random.default_rng(5).permutation(M).astype(U32)
    hub = int(perm[0])
    parent = np.full(M, hub, dtype=U32)
    parent[hub] = POOL_ROOT
    depth = np.full(M, 2, dtype=U32)
    depth[hub] = 1
    F = du.SimpleNamespace(parent=parent, depth=depth, n=M)
    check_tips(gpu, F, "star of 2^20")
    leaves = [int(x) for x in perm[1:8]]

    def want(index, n_bad):
        on = np.ones(M, dtype=np.uint8)
        everyone = np.ones(M, dtype=bool)
        single = [au.key_of(index, n_bad, np.arange(M) == x) for x in leaves]
        return [M] + [1] * 7, [1] + [0] * 7, [au.key_of(index, n_bad, everyone)] + single, on
    check_subtrees(gpu, F, [hub] + leaves, want, "star of 2^20")
    on = np.zeros(M, dtype=np.uint8)
    on[leaves] = 1
    check_drop(gpu, F, leaves + leaves[:2], on, "star of 2^20, seven leaves dropped")
    check_drop(gpu, F, [hub], np.ones(M, dtype=np.uint8), "star of 2^20, everything dropped")


# ---- the two-arm shape ----
def test_two_arms(gpu):
    T = du.two_arms(300_000, 400_000, 348_576 - 100, 9)
    a_low, b_low = int(T.line_a[T.trunk]), int(T.line_b[T.trunk])
    roots = [T.top, a_low, b_low, int(T.line_a[-1]), int(T.line_a[0]), int(T.line_b[T.trunk + 1000])]

    def want(index, n_bad):
        sets = [T.depth >= T.trunk, T.side == 1, T.side == 2, np.arange(T.n) == roots[3], np.ones(T.n, dtype=bool),
                (T.side == 2) & (T.depth >= T.trunk + 1001)]
        on = np.ones(T.n, dtype=np.uint8)
        return ([int(m.sum()) for m in sets], [int(T.depth[m].max()) - int(T.depth[r]) for m, r in zip(sets, roots)],
                [au.key_of(index, n_bad, m) for m in sets], on)
    n_bad = (np.arange(T.n, dtype=U32) % 7 == 1).astype(U32)
    check_subtrees(gpu, T, roots, want, "two arms", n_bad=n_bad, index=(np.arange(T.n, dtype=U32) * 2654435761 >> 7).astype(U32))
    check_drop(gpu, T, [b_low], (T.side == 2).astype(np.uint8), "two arms, the losing arm dropped")
    check_drop(gpu, T, [a_low, b_low], (T.side != 0).astype(np.uint8), "two arms, both dropped", fin=1)
    check_tips(gpu, T, "two arms")


# ---- 64 roots at 2^16 nodes ----
def test_64_roots_at_2_16(gpu):
    F = du.random_forest(1 << 16, 31)
    rng = np.random.default_rng(3)
    roots = [int(F.hidden[0])] + [int(F.hidden[x]) for x in rng.integers(1, 200, 40)] + rng.integers(0, F.n, 21).tolist()
    roots += roots[:2]
    assert len(roots) == 64
    n_bad = (rng.integers(0, 4, F.n) == 0).astype(U32)
    index = rng.integers(0, 50, F.n).astype(U32)  # many ties: the lowest position wins
    check_subtrees(gpu, F, roots, lambda i, b: au.subtrees_of(F.parent, F.depth, i, b, roots), "64 roots", index=index, n_bad=n_bad)
    few = roots[5:12]
    check_drop(gpu, F, few, au.subtrees_of(F.parent, F.depth, index, n_bad, few)[3], "forest of 2^16")
    check_tips(gpu, F, "forest of 2^16")
    check_tips(gpu, F, "forest of 2^16, the other scratch half", fin=1)


# ---- sizes around the seams of the count and the gather ----
@pytest.mark.parametrize("n", [1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097])
def test_ragged_sizes(gpu, n):
    """n % 4 != 0 leaves a tail in the last mark word, which K12c counts: the keep-marks' preset must not reach it."""
    F = du.random_forest(n, n)
    check_tips(gpu, F, f"forest of {n}")
    roots = [int(F.hidden[0]), int(F.hidden[n // 2]), int(F.hidden[n - 1])]
    index = np.arange(n, dtype=U32) % 11
    n_bad = (np.arange(n, dtype=U32) % 4 == 2).astype(U32)
    want = au.subtrees_of(F.parent, F.depth, index, n_bad, roots)
    check_subtrees(gpu, F, roots, lambda i, b: want, f"forest of {n}", index=index, n_bad=n_bad)
    for fin in (0, 1):
        check_drop(gpu, F, roots[1:], au.subtrees_of(F.parent, F.depth, index, n_bad, roots[1:])[3], f"forest of {n}", fin=fin)


def test_the_hook_checks_its_arguments(gpu):
    L = du.shuffled_list(10, 1)
    zeros = np.zeros(10, dtype=U32)
    for roots in ((), (10,), tuple(range(10)) * 7):
        rc, _ = au.run_above(gpu.L, gpu.ctx, L.parent, L.depth, zeros, zeros, SUBTREES, roots)
        assert rc == POW_EINVAL, roots
    rc, _ = au.run_above(gpu.L, gpu.ctx, L.parent, L.depth, zeros, zeros, TIPS, (), flags=2)
    assert rc == POW_EINVAL and "unknown flags" in last_error(gpu.L)
