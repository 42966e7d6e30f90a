"""K12 and K13 on the GPU on synthetic forests of up to 2^20 nodes (the pool's
limit), through the test library's pow_test_pool_prune and pow_test_pool_lift:
the cross-wave half of K12d's scan (first used at 1,025 partials), K12b's
rounds 18 to 20, K12c, K12e and K12f over up to 4,096 workgroups, K13's levels
12 to 19 and the chain call at 2^20 lanes.  The forests are numpy arrays with
closed-form answers (tests/pool_deep_util.py, held against plain walks by
tests/test_pool_deep_host.py); nothing is hashed.  Every comparison is exact.
One small case per hook also goes through the public pool calls on real blocks.

Wall time per case on an MI355X: the mark patterns 0.08 to 0.62 s (random marks
over 22 sizes the slowest, mod257 0.41 s), sound_only 0.22 s, fork_choice 0.15
and 0.21 s, the tables at 2^20 0.05 to 0.13 s, the lists of 2^20 0.10 s, the
extensions at 2^20 0.07 to 0.10 s, every other case 0.05 s or less; 7.6 s for
the file, 1.6 s of it the context's setup."""
import numpy as np
import pytest

from mpi_blockchain_amd._lib import POW_EINVAL
from mpi_blockchain_amd.block import POOL_NONE, POOL_ROOT
from mpi_blockchain_amd.miner import GpuMiner

import pool_deep_util as du
import pool_util as pu
from pool_deep_util import ANCESTORS, CHAIN, FORKS, KEEP_BY_INDEX, KEEP_SOUND_ONLY
from test_pool_lift_gpu import lift_launches, rows

pytestmark = pytest.mark.gpu

U32 = np.uint32
M = 1 << 20
ALL_ONES = 0xFFFFFFFF


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


def prune(gpu, F, tips=(), min_index=0, flags=0, fin=0):
    rc, o = du.run_prune(gpu.L, gpu.ctx, F, tips, min_index, flags, fin)
    assert rc == 0, last_error(gpu.L)
    return o


def lift(gpu, parent, depth, mode=ANCESTORS, **kw):
    rc, o = du.run_lift(gpu.L, gpu.ctx, parent, depth, mode, **kw)
    assert rc == 0, last_error(gpu.L)
    return o


def same(got, want, what):
    """Exact equality of two arrays, with the first difference in the message."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        at = int(np.flatnonzero(got.reshape(-1) != want.reshape(-1))[0])
        raise AssertionError(f"{what}: {int((got != want).sum())} entries differ, the first at {at}: "
                             f"{got.reshape(-1)[at]} for {want.reshape(-1)[at]}")


def check_prune(o, F, marks, what):
    """Everything the hook gives against the reference of a prune that keeps `marks`."""
    same(o.marks, marks, f"{what}: marks")
    want = du.pruned(F, marks)
    assert o.kept == want.kept, (what, o.kept, want.kept)
    if want.kept == F.n:  # nothing dropped: K12a's positions, the arrays as they were, no new control words
        same(o.map, np.arange(F.n, dtype=U32), f"{what}: map")
        for name in ("parent", "index", "depth", "n_bad", "status", "digest", "prev"):
            same(getattr(o, name), getattr(F, name), f"{what}: {name}")
        assert (o.best, o.n_flagged) == (0, 0), what
        return want
    same(o.map, want.map, f"{what}: map")
    for name in ("parent", "index", "depth", "n_bad", "status", "digest", "prev"):
        same(getattr(o, name), getattr(want, name), f"{what}: {name}")
    assert (o.best, o.n_flagged) == (want.best, want.n_flagged), (what, hex(o.best), hex(want.best), o.n_flagged, want.n_flagged)
    return want


# ---- K12c to K12e: mark patterns with no tree ----
def sizes(ps, rs=(0, 255)):
    return [256 * p - r for p in ps for r in rs]


EVERY = sizes((1, 16, 17, 1023, 1024, 1025, 2049, 3072, 3073, 4095, 4096))
SEAMS = sizes((1, 17, 1024, 1025, 4096))  # a subset with the sizes around 1,024 and 4,096 partials


def pattern(kind: str, n: int):
    pos = np.arange(n)
    part, off = pos >> 8, pos & 255
    if kind == "all":
        return np.ones(n, dtype=np.uint8)
    if kind == "none":
        return np.zeros(n, dtype=np.uint8)
    if kind == "first":
        return (pos == 0).astype(np.uint8)
    if kind == "last":
        return (pos == n - 1).astype(np.uint8)
    if kind == "one_per_partial":  # at a rotating offset; the ragged last partial may hold none
        return (off == (part * 7) % 256).astype(np.uint8)
    if kind == "mod257":  # partial p holds (37 p) mod 257 marks, from a rotating offset on
        return (((off - part) % 256) < (37 * part) % 257).astype(np.uint8)
    if kind == "random":
        return np.random.default_rng(n).integers(0, 2, n).astype(np.uint8)
    q = int(kind[-1])  # quarter q: exactly the partials 1024 q .. 1024 q + 1023 are full
    return ((part >> 10) == q).astype(np.uint8)


PATTERNS = {"all": SEAMS, "none": SEAMS, "first": SEAMS, "last": SEAMS, "one_per_partial": EVERY, "mod257": EVERY,
            "random": EVERY, "quarter0": sizes((2049, 3073, 4095, 4096)), "quarter1": sizes((2049, 3073, 4095, 4096)),
            "quarter2": sizes((2049, 3073, 4095, 4096)), "quarter3": sizes((3073, 4095, 4096))}


@pytest.mark.parametrize("kind", sorted(PATTERNS))
def test_scan_and_gather_over_mark_patterns(gpu, kind):
    for n in PATTERNS[kind]:
        marks = pattern(kind, n)
        if kind == "mod257":  # the pattern is what it says: no two wave sums or lane sums of K12d coincide by design
            full = du.partials_of(marks)[:n // 256]
            assert full.tolist() == [(37 * p) % 257 for p in range(n // 256)]
        F = du.marks_by_index(marks)
        o = prune(gpu, F, (), F.min_index, F.flags, fin=n & 1)
        want = check_prune(o, F, marks, f"{kind}, {n} nodes")
        assert want.kept == int(marks.sum())
        if kind.startswith("quarter"):
            assert want.kept == max(0, min(n, 262144 * (int(kind[-1]) + 1)) - 262144 * int(kind[-1]))


# ---- K12a and K12b at depth ----
def forest_of(T, **entries):
    return du.SimpleNamespace(n=T.n, parent=T.parent, **vars(du.payload(T.n, depth=T.depth, **entries)))


@pytest.mark.parametrize("n", [(1 << 17) + 3, 1 << 19, (1 << 19) + 1, M - 1, M])
def test_marks_reach_the_root_of_a_long_list(gpu, n):
    """rounds(n) rounds of K12b carry one seed's mark down n - 1 steps: one
    round fewer leaves the root unmarked."""
    L = du.shuffled_list(n, n % 1000)
    F = forest_of(L)
    tip = int(L.order[-1])
    o = prune(gpu, F, [tip])
    assert o.marks[L.order[0]] == 1, "the root is unmarked"
    check_prune(o, F, np.ones(n, dtype=np.uint8), f"the tip of {n}")
    # the seed two steps under the tip: exactly the two top nodes go, wherever they lie
    marks = np.ones(n, dtype=np.uint8)
    marks[L.order[-2:]] = 0
    o = prune(gpu, F, [int(L.order[-3])], fin=1)
    assert o.marks[L.order[0]] == 1, "the root is unmarked"
    want = check_prune(o, F, marks, f"two under the tip of {n}")
    assert want.kept == n - 2 and sorted(np.flatnonzero(o.map == POOL_NONE).tolist()) == sorted(L.order[-2:].tolist())


def test_the_most_tips_on_a_ragged_list(gpu):
    """2^16 tips on 2^20 - 1 nodes: the tips' lanes of K12a start in the middle of a workgroup."""
    n = M - 1
    L = du.shuffled_list(n, 7)
    F = forest_of(L)
    heights = np.random.default_rng(5).integers(0, 3 * n // 4, du.MAX_TIPS)
    marks = np.zeros(n, dtype=np.uint8)
    marks[L.order[:int(heights.max()) + 1]] = 1
    o = prune(gpu, F, L.order[heights])
    want = check_prune(o, F, marks, "2^16 tips")
    assert 0 < want.kept < n


def test_a_dead_arm_is_dropped(gpu):
    T = du.two_arms(1 << 19, 1 << 18, (1 << 18) - 1, 3)
    rng = np.random.default_rng(8)
    F = forest_of(T, status=(rng.random(T.n) < 0.03), index=rng.integers(1, 1 << 30, T.n))
    o = prune(gpu, F, [int(T.line_a[-1])])
    want = check_prune(o, F, (T.side != 2).astype(np.uint8), "arm A's tip")
    assert want.kept == (1 << 19) + (1 << 18) and (o.map[T.line_b[T.trunk:]] == POOL_NONE).all()
    # the survivors' parents by the new positions, the root staying a root
    assert o.parent[o.map[T.line_a[0]]] == POOL_ROOT and (o.parent == POOL_ROOT).sum() == 1
    same(o.parent[o.map[T.line_a[1:]]], o.map[T.line_a[:-1]], "the line's parents")
    assert want.n_flagged == int((F.status[T.side != 2] != 0).sum()) > 20000


def test_sound_only_on_a_wide_forest(gpu):
    n = M - 5
    T = du.random_forest(n, 12)
    rng = np.random.default_rng(13)
    n_bad = (rng.random(n) < 0.01).astype(U32) * rng.integers(1, 9, n).astype(U32)
    F = forest_of(T, index=rng.integers(0, 1000, n), n_bad=n_bad, status=(rng.random(n) < 0.03) * rng.integers(1, 16, n))
    tips = rng.integers(0, n, 100)
    by_index = np.flatnonzero(F.index >= 990)
    sound = by_index[n_bad[by_index] == 0]
    assert 50 < len(by_index) - len(sound) < 300
    marks = du.marks_of(T.parent, T.depth, np.concatenate([sound, tips]))
    loose = du.marks_of(T.parent, T.depth, np.concatenate([by_index, tips]))
    assert marks.sum() < loose.sum() < n // 2  # the flag matters here
    o = prune(gpu, F, tips, 990, KEEP_BY_INDEX | KEEP_SOUND_ONLY)
    check_prune(o, F, marks, "sound only")
    o = prune(gpu, F, tips, 990, KEEP_BY_INDEX, fin=1)
    check_prune(o, F, loose, "by index")
    o = prune(gpu, F, tips, 990, KEEP_SOUND_ONLY)  # without POW_KEEP_BY_INDEX the index rule is off
    check_prune(o, F, du.marks_of(T.parent, T.depth, tips), "tips only")


# ---- K12f at scale ----
@pytest.mark.parametrize("shape", ["list", "arms"])
def test_fork_choice_over_every_workgroup(gpu, list20, shape):
    """The greatest index three times among the survivors, in workgroups far
    apart: the lowest position wins; a greater one on an unsound survivor does
    not count; the flagged count over a random 3 %."""
    if shape == "list":
        T, seed = list20, int(list20.order[-3])
        marks = np.ones(M, dtype=np.uint8)
        marks[list20.order[-2:]] = 0
    else:
        T = du.two_arms(1 << 19, 1 << 18, (1 << 18) - 1, 3)
        seed, marks = int(T.line_a[-1]), (T.side != 2).astype(np.uint8)
    rng = np.random.default_rng(21)
    kept, new = du.map_of(marks)
    alive = np.flatnonzero(marks)
    index = rng.integers(1, 1000, T.n)
    n_bad = np.zeros(T.n, dtype=U32)
    ties = alive[[kept - 7, kept // 3, kept // 3 + 1500, 3000]]  # new positions kept - 7, ..., 3000: the last named is the lowest
    index[ties] = 5000
    liar = alive[1200]  # a lower position still, and a greater index, but unsound
    index[liar], n_bad[liar] = 6000, 1
    n_bad[alive[rng.integers(0, kept, 5000)]] = 2
    n_bad[ties] = 0
    status = (rng.random(T.n) < 0.03) * rng.integers(1, 256, T.n)
    F = forest_of(T, index=index, n_bad=n_bad, status=status)
    o = prune(gpu, F, [seed])
    want = check_prune(o, F, marks, shape)
    assert want.best == (5000 << 32) | (~3000 & ALL_ONES) and o.best == want.best
    assert o.n_flagged == int((status[alive] != 0).sum()) > 20000
    # every tie unsound but the one in the last workgroup: that one wins, and the liar still does not count
    F.n_bad = n_bad.copy()
    F.n_bad[ties[1:]] = 1
    o = prune(gpu, F, [seed])
    want = check_prune(o, F, marks, shape)
    assert o.best == (5000 << 32) | (~(kept - 7) & ALL_ONES)
    # nobody sound: no best
    F.n_bad = np.ones(T.n, dtype=U32)
    o = prune(gpu, F, [seed])
    check_prune(o, F, marks, shape)
    assert o.best == 0


# ---- K13: the table ----
TABLE_SIZES = [(1 << 11) + 1, (1 << 16) + 1, 1 << 19, (1 << 19) + 1, M]


@pytest.mark.parametrize("capacity", ["n", "2^20"])
@pytest.mark.parametrize("n", TABLE_SIZES)
def test_table_of_a_list_from_nothing(gpu, n, capacity):
    L = du.shuffled_list(n, n % 999, end=POOL_NONE if n & 1 else POOL_ROOT)
    o = lift(gpu, L.parent, L.depth, k=0, capacity=n if capacity == "n" else M, table=True)
    assert o.launches == rows(n) == lift_launches(0, n, True) == len(o.table)
    for j in range(1, rows(n) + 1):
        same(o.table[j - 1], du.list_row(L, j), f"row {j} of {n}")


@pytest.mark.parametrize("capacity", ["n", "2^20"])
@pytest.mark.parametrize("n", TABLE_SIZES)
def test_table_of_a_forest_from_nothing(gpu, n, capacity):
    T = du.random_forest(n, n % 997)
    o = lift(gpu, T.parent, T.depth, k=0, capacity=n if capacity == "n" else M, table=True)
    assert o.launches == rows(n) == lift_launches(0, n, True)
    for j, want in enumerate(du.doubling_rows(T.parent, rows(n)), 1):
        same(o.table[j - 1], want, f"row {j} of {n}")
    for i in np.random.default_rng(n).integers(0, n, 200).tolist():  # plain walks over a sample
        walk, end = du.plain_walk(T.parent, i)
        assert len(walk) == T.depth[i]
        assert o.table[:, i].tolist() == [walk[1 << j] if (1 << j) < len(walk) else end for j in range(1, rows(n) + 1)]


EXTENSIONS = [((1 << 16), (1 << 16) + 1), ((1 << 16) + 1 - 256, (1 << 16) + 1), ((1 << 16) + 1 - 257, (1 << 16) + 1),
              (M - 2, M - 1), (M - 1 - 256, M - 1), (M - 1 - 257, M - 1),
              ((1 << 19) - 100, (1 << 19) + 100), (1 << 19, (1 << 19) + 1), (M - 256, M)]


@pytest.mark.parametrize("covered,n", EXTENSIONS)
def test_table_extended_over_a_linked_batch(gpu, covered, n):
    """The new nodes are a run linked inside the batch and shuffled among
    themselves, on top of a list over the covered ones: K13b (at most 256) or
    K13a per row, then the rows that are new, give the table made from nothing."""
    L = du.shuffled_list(n, covered % 991, covered=covered)
    capacity = n if covered & 1 else M
    fresh = lift(gpu, L.parent, L.depth, k=0, capacity=capacity, table=True)
    fed = lift(gpu, L.parent, L.depth, k=0, capacity=capacity, covered=covered, table=True)
    assert fed.launches == lift_launches(covered, n, False), (fed.launches, covered, n)
    assert fed.launches == ((1 if n - covered <= 256 else rows(covered)) + rows(n) - rows(covered))
    same(fed.table, fresh.table, f"extended from {covered} to {n}")
    for j in range(1, rows(n) + 1):
        same(fed.table[j - 1], du.list_row(L, j), f"row {j} of {n}")


# ---- K13c ----
@pytest.mark.parametrize("k", [M, M - 1, 257, 1])
def test_chain_of_the_longest_list(gpu, list20, k):
    """The chain of the tip is the list reversed: every step count 0 .. k - 1 in one launch."""
    tip = int(list20.order[-1])
    o = lift(gpu, list20.parent, list20.depth, CHAIN, tip=tip, k=k)
    want, length = du.list_chain(list20, tip, k)
    assert o.length == length == k and o.launches == 19
    same(o.out, want, f"chain of {k}")
    same(o.out, list20.order[::-1][:k], f"chain of {k}")


def test_chain_of_an_orphans_list_and_from_its_middle(gpu):
    n = (1 << 19) + 1
    L = du.shuffled_list(n, 31, end=POOL_NONE)
    tip, mid = int(L.order[-1]), int(L.order[(1 << 18) + 5])
    o = lift(gpu, L.parent, L.depth, CHAIN, tip=tip, k=n, capacity=M)
    assert o.length == n
    same(o.out, L.order[::-1], "the orphan's chain")
    o = lift(gpu, L.parent, L.depth, CHAIN, tip=mid, k=n)  # shorter than asked for: POOL_NONE behind the walk
    assert o.length == (1 << 18) + 6
    same(o.out[:o.length], L.order[:o.length][::-1], "from the middle")
    assert (o.out[o.length:] == POOL_NONE).all()
    q = lift(gpu, L.parent, L.depth, ANCESTORS, in0=[tip, tip, tip, mid], in1=[n - 1, n, ALL_ONES, o.length])
    assert q.out.tolist() == [int(L.order[0]), POOL_NONE, POOL_NONE, POOL_NONE]


def step_counts(depth: int):
    s = {0, 1, depth - 1, depth, depth + 1, ALL_ONES}
    for j in range(21):
        s |= {(1 << j) - 1, 1 << j, (1 << j) + 1}
    return sorted(s)


def test_ancestors_at_every_power_of_two(gpu, list20):
    rng = np.random.default_rng(17)
    starts = [M, M - 1, (1 << 19) + 1, 1 << 19, 1] + rng.integers(1, M + 1, 300).tolist()  # heights
    pos, steps = [], []
    for h in starts:
        for s in step_counts(h):
            pos.append(int(list20.order[h - 1]))
            steps.append(s)
    o = lift(gpu, list20.parent, list20.depth, ANCESTORS, in0=pos, in1=steps)
    same(o.out, du.list_ancestor(list20, pos, steps), "ancestors")
    assert o.out[steps.index(M - 1)] == list20.order[0] and o.out[steps.index(M)] == POOL_ROOT  # from the tip
    assert len(pos) > 15000


@pytest.mark.parametrize("n", [(1 << k) + e for k in (7, 11, 12, 16, 19, 20) for e in (0, 1) if (1 << k) + e <= M])
def test_depth_equal_to_two_to_the_levels(gpu, n, list20):
    """A list of exactly 2^k nodes has k levels and a walk of 2^k blocks: the
    walk to the end applies the bits of depth - 1.  2^k + 1 has one level more."""
    L = list20 if n == M else du.shuffled_list(n, n % 77)
    tip = int(L.order[-1])
    steps = [0, 1, n // 2 - 1, n // 2, n // 2 + 1, n - 2, n - 1, n, n + 1, ALL_ONES]
    pos = [tip] * len(steps) + [int(L.order[-2])] * len(steps) + [int(L.order[n // 2])] * len(steps)
    o = lift(gpu, L.parent, L.depth, ANCESTORS, in0=pos, in1=steps * 3, capacity=M if n & 1 else n)
    same(o.out, du.list_ancestor(L, pos, steps * 3), f"list of {n}")
    assert o.out[:len(steps)].tolist()[-4:] == [int(L.order[0]), POOL_ROOT, POOL_ROOT, POOL_ROOT]
    assert o.launches == rows(n)
    c = lift(gpu, L.parent, L.depth, CHAIN, tip=tip, k=n)
    assert c.length == n
    same(c.out, L.order[::-1], f"chain of {n}")


# ---- K13d ----
ARMS = [(1 << 19, 1 << 18, (1 << 18) - 1), (1, 1 << 19, (1 << 19) - 2), ((1 << 19) + 1, 1, (1 << 19) - 2), (M - 2, 1, 1)]


def arm_pairs(T, k: int, seed: int):
    """k pairs: across the arms at heights 1, 2^j and the arms' lengths, on one
    line, a == b, a node and its parent; filled up with random pairs."""
    a_arm, b_arm = T.line_a[T.trunk:], T.line_b[T.trunk:]
    heights = lambda arm: sorted({h for j in range(21) for h in ((1 << j) - 1, 1 << j, (1 << j) + 1) if 1 <= h <= len(arm)}
                                 | {len(arm)})
    tip_a, tip_b, under_a = int(a_arm[-1]), int(b_arm[-1]), int(T.line_a[-2])
    first = [(tip_a, tip_b), (tip_b, tip_b), (tip_a, under_a), (under_a, tip_a), (tip_b, tip_a), (T.top, T.top)]
    across, one_line = [], []
    for ha in heights(a_arm):
        for hb in heights(b_arm):
            across += [(int(a_arm[ha - 1]), int(b_arm[hb - 1])), (int(b_arm[hb - 1]), int(a_arm[ha - 1]))]
    for line in (T.line_a, T.line_b):
        for h in heights(line):
            one_line += [(int(line[-1]), int(line[h - 1])), (int(line[h - 1]), int(line[0])), (int(line[h - 1]), int(line[h - 1]))]
            if h > 1:
                one_line += [(int(line[h - 1]), int(line[h - 2])), (int(line[h - 2]), int(line[h - 1]))]
    rng = np.random.default_rng(seed)
    rng.shuffle(across)
    rng.shuffle(one_line)
    pairs = first + one_line[:k // 3] + across[:k // 3] + one_line[k // 3:] + across[k // 3:]
    pairs = pairs[:k] + [(int(x), int(y)) for x, y in rng.integers(0, T.n, (max(k - len(pairs), 0), 2))]
    return np.array(pairs, dtype=U32)


@pytest.mark.parametrize("k", [1, 257, (1 << 16) + 1])
@pytest.mark.parametrize("trunk,a,b", ARMS)
def test_fork_points_of_two_arms(gpu, trunk, a, b, k):
    T = du.two_arms(trunk, a, b, trunk % 13)
    pairs = arm_pairs(T, k, k)  # the first is the two tips
    o = lift(gpu, T.parent, T.depth, FORKS, in0=pairs[:, 0], in1=pairs[:, 1], capacity=M if k == 257 else T.n)
    at, back_a, back_b = du.arms_fork(T, pairs[:, 0], pairs[:, 1])
    same(o.out[0], at, "at")
    same(o.out[1], back_a, "back_a")
    same(o.out[2], back_b, "back_b")
    assert (int(o.out[0][0]), int(o.out[1][0]), int(o.out[2][0])) == (T.top, a, b)
    if k > 1:  # a == b, a node against its parent both ways, the trunk's top against itself
        assert [(int(o.out[0][q]), int(o.out[1][q]), int(o.out[2][q])) for q in range(1, 6)] == \
            [(pairs[1][0], 0, 0), (pairs[3][0], 1, 0), (pairs[3][0], 0, 1), (T.top, b, a), (T.top, 0, 0)]
    assert o.launches == rows(T.n)


@pytest.mark.parametrize("k", [1, 257, (1 << 16) + 1])
def test_no_fork_point_between_two_lists(gpu, k):
    T = du.two_lists(1 << 19, (1 << 19) - 3, 41)
    rng = np.random.default_rng(k)
    a = T.line_a[rng.integers(0, len(T.line_a), k)]
    b = T.line_b[rng.integers(0, len(T.line_b), k)]
    a[0], b[0] = T.line_a[-1], T.line_b[-1]
    flip = rng.random(k) < 0.5
    x, y = np.where(flip, b, a), np.where(flip, a, b)
    o = lift(gpu, T.parent, T.depth, FORKS, in0=x, in1=y)
    assert (o.out[0] == POOL_NONE).all()
    same(o.out[1], T.depth[x], "back_a: the depth")
    same(o.out[2], T.depth[y], "back_b: the depth")
    same(lift(gpu, T.parent, T.depth, FORKS, in0=a, in1=a).out[0], a, "a == a")


# ---- one small case per hook through the public pool calls as well ----
@pytest.fixture(scope="module")
def tree():
    return pu.tree(seed=3)


@pytest.mark.parametrize("seeds", [([25, 39], None, False), ([31], 12, False), ([], 10, True), ([12, 25, 31, 39], 0, False)])
def test_the_prune_hook_agrees_with_the_pool(gpu, tree, seeds):
    tips, min_index, sound_only = seeds
    flags = 0 if min_index is None else KEEP_BY_INDEX | (KEEP_SOUND_ONLY if sound_only else 0)
    with gpu.open_pool(pu.D) as pool:
        pool.add(tree)
        r = pool.read()
        index = np.array([b.index for b in tree], dtype=U32)
        F = du.SimpleNamespace(n=40, parent=r.parent, **vars(du.payload(40, index=index, n_bad=r.n_bad, status=r.status, depth=r.depth)))
        o = prune(gpu, F, tips, min_index or 0, flags)
        same(o.marks, pool.mark(tips, min_index, sound_only), "marks")
        new, info = pool.prune(tips, min_index, sound_only)
        same(o.map, new, "map")
        after = pool.read()
        assert o.kept == info["size"] == len(after.parent)
        for got, want in ((o.parent, after.parent), (o.depth, after.depth), (o.n_bad, after.n_bad), (o.status, after.status)):
            same(got, want, "the survivors")
        if o.kept < 40:
            assert o.n_flagged == info["n_flagged"]
            assert (None if o.best == 0 else ~o.best & ALL_ONES, o.best >> 32) == (info["best"], info["best_index"])
        check_prune(o, F, o.marks, "the tree")


def test_the_lift_hook_agrees_with_the_pool(gpu, tree):
    with gpu.open_pool(pu.D) as pool:
        pool.add(tree[:31])
        r = pool.read()
        pairs = np.array([(a, b) for a in range(31) for b in range(31)], dtype=U32)
        want = pool.fork_points(pairs[:, 0], pairs[:, 1])
        assert gpu.stats()["launches"] == rows(31) + 1
        o = lift(gpu, r.parent, r.depth, FORKS, in0=pairs[:, 0], in1=pairs[:, 1], capacity=64)
        assert o.launches == rows(31)
        for got, ref in zip(o.out, want):
            same(got, ref, "fork points")
        # nine more blocks: the pool extends its table, and so does the hook
        pool.add(tree[31:])
        r = pool.read()
        pos = np.repeat(np.arange(40, dtype=U32), 20)
        steps = np.tile(np.array(list(range(19)) + [ALL_ONES], dtype=U32), 40)
        want = pool.ancestors(pos, steps)
        assert gpu.stats()["launches"] == lift_launches(31, 40, False) + 1
        o = lift(gpu, r.parent, r.depth, ANCESTORS, in0=pos, in1=steps, capacity=64, covered=31, table=True)
        assert o.launches == lift_launches(31, 40, False)
        same(o.out, want, "ancestors")
        same(o.table, lift(gpu, r.parent, r.depth, k=0, capacity=64, table=True).table, "the table")
        for tip in (12, 25, 39):
            c = lift(gpu, r.parent, r.depth, CHAIN, tip=tip, k=40)
            same(c.out[:c.length], pool.chain(tip), "chain")
            assert c.length == r.depth[tip] and (c.out[c.length:] == POOL_NONE).all()


def test_refusals_leave_the_context_usable(gpu):
    """One POW_EINVAL per hook on a live context, then a call that passes (the
    cases themselves: tests/test_pool_deep_host.py)."""
    L = du.shuffled_list(300, 2)
    rc, _ = du.run_prune(gpu.L, gpu.ctx, forest_of(L), tips=[300])
    assert rc == POW_EINVAL and "tip 0 (node 300) past the forest's 300" in last_error(gpu.L)
    rc, _ = du.run_lift(gpu.L, gpu.ctx, L.parent, L.depth, CHAIN, tip=300, k=3)
    assert rc == POW_EINVAL and "tip (node 300)" in last_error(gpu.L)
    nothing = du.SimpleNamespace(n=0, parent=np.zeros(0, dtype=U32), **vars(du.payload(0)))
    assert du.run_prune(gpu.L, gpu.ctx, nothing)[0] == 0  # no nodes: nothing to do
    o = lift(gpu, L.parent, L.depth, CHAIN, tip=int(L.order[-1]), k=300)
    same(o.out, L.order[::-1], "chain")
