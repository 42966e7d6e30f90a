"""The deep pool tests' instruments on the host (CPU only): the generators and
references of tests/pool_deep_util.py at a few hundred nodes against plain
walks written out here; the two hooks pow_test_pool_prune and
pow_test_pool_lift in the test library only; and their POW_EINVAL cases, which
need no GPU: every check stands in front of the first use of the context."""
import ctypes
import os
import re

import numpy as np
import pytest

from mpi_blockchain_amd import _lib
from mpi_blockchain_amd.block import POOL_NONE, POOL_ROOT

import pool_deep_util as du

HOOKS = ("pow_test_pool_prune", "pow_test_pool_lift")


def walk(parent, pos):
    out = []
    while pos < len(parent):
        out.append(int(pos))
        pos = int(parent[pos])
        assert len(out) <= len(parent)
    return out, pos


def check_forest(parent, depth):
    ends = set()
    for i in range(len(parent)):
        w, end = walk(parent, i)
        assert depth[i] == len(w)
        ends.add(end)
    return ends


# ---- the generators ----
@pytest.mark.parametrize("n,end,covered", [(1, POOL_ROOT, 0), (2, POOL_NONE, 0), (257, POOL_ROOT, 0), (300, POOL_NONE, 0),
                                           (300, POOL_ROOT, 44), (300, POOL_ROOT, 299)])
def test_shuffled_list(n, end, covered):
    L = du.shuffled_list(n, 5, end, covered)
    assert sorted(L.order.tolist()) == list(range(n)) and check_forest(L.parent, L.depth) == {end}
    tip = int(L.order[-1])
    w, _ = walk(L.parent, tip)
    assert w == L.order[::-1].tolist()
    if n > 2:
        assert w != sorted(w) and w != sorted(w, reverse=True)  # shuffled
    assert sorted(L.order[:covered].tolist()) == list(range(covered))
    assert all(p < covered or p == end for p in L.parent[:covered].tolist())  # closed under parent
    for pos in range(n):
        w, _ = walk(L.parent, pos)
        steps = list(range(len(w) + 2)) + [0xFFFFFFFF]
        assert du.list_ancestor(L, [pos] * len(steps), steps).tolist() == [w[s] if s < len(w) else end for s in steps]
        for k in (0, 1, 3, len(w), len(w) + 1, n):
            got, length = du.list_chain(L, pos, k)
            assert got.tolist() == w[:k] and length == min(len(w), k)
    for j in range(0, 10):
        want = [w[1 << j] if (1 << j) < len(w) else end for w in (walk(L.parent, i)[0] for i in range(n))]
        assert du.list_row(L, j).tolist() == want
    assert du.list_row(L, 0).tolist() == L.parent.tolist()


@pytest.mark.parametrize("trunk,a,b", [(1, 1, 1), (5, 3, 4), (100, 50, 49), (1, 120, 118), (130, 1, 120), (200, 1, 1)])
def test_two_arms(trunk, a, b):
    T = du.two_arms(trunk, a, b, 9)
    assert T.n == trunk + a + b and check_forest(T.parent, T.depth) == {POOL_ROOT}
    assert walk(T.parent, int(T.line_a[-1]))[0] == T.line_a[::-1].tolist()
    assert walk(T.parent, int(T.line_b[-1]))[0] == T.line_b[::-1].tolist()
    assert T.line_a[:trunk].tolist() == T.line_b[:trunk].tolist() and T.top == T.line_a[trunk - 1]
    assert not set(T.line_a[trunk:].tolist()) & set(T.line_b[trunk:].tolist())
    assert (T.side[T.line_a[trunk:]] == 1).all() and (T.side[T.line_b[trunk:]] == 2).all() and (T.side != 0).sum() == a + b
    rng = np.random.default_rng(1)
    xs, ys = rng.integers(0, T.n, 600), rng.integers(0, T.n, 600)
    xs[:3], ys[:3] = (T.line_a[-1], T.line_b[-1], T.top), (T.line_b[-1], T.line_b[-1], T.line_a[-1])
    at, ba, bb = du.arms_fork(T, xs, ys)
    assert list(zip(at.tolist(), ba.tolist(), bb.tolist())) == [du.plain_fork(T.parent, int(x), int(y)) for x, y in zip(xs, ys)]
    assert (at[0], ba[0], bb[0]) == (T.top, a, b)


def test_two_lists():
    T = du.two_lists(130, 77, 4)
    assert check_forest(T.parent, T.depth) == {POOL_ROOT, POOL_NONE}
    assert walk(T.parent, int(T.line_a[-1])) == (T.line_a[::-1].tolist(), POOL_ROOT)
    assert walk(T.parent, int(T.line_b[-1])) == (T.line_b[::-1].tolist(), POOL_NONE)
    for x in T.line_a[::13].tolist():
        for y in T.line_b[::7].tolist():
            assert du.plain_fork(T.parent, x, y) == (POOL_NONE, T.depth[x], T.depth[y])


@pytest.mark.parametrize("n", [1, 2, 700, 5000])
def test_random_forest(n):
    F = du.random_forest(n, 6)
    ends = check_forest(F.parent, F.depth)  # depths_of against plain walks
    assert sorted(F.hidden.tolist()) == list(range(n)) and F.parent[F.hidden[0]] == POOL_ROOT
    if n >= 5000:
        assert ends == {POOL_ROOT, POOL_NONE} and 4 < F.depth.max() < 64  # shallow, with orphans and several roots
        assert (F.parent >= n).sum() > 3
    where = np.empty(n, dtype=np.int64)
    where[F.hidden] = np.arange(n)
    inner = F.parent < n
    assert (where[F.parent[inner]] < where[inner]).all()  # every parent earlier in the hidden order
    table = du.doubling_rows(F.parent, 4)
    for i in range(0, n, 7):
        w, end = walk(F.parent, i)
        for j in range(1, 5):
            assert table[j - 1][i] == (w[1 << j] if (1 << j) < len(w) else end)


# ---- K12's references ----
def test_marks_of_against_plain_walks():
    F = du.random_forest(3000, 8)
    rng = np.random.default_rng(2)
    for seeds in ([], [5], rng.integers(0, 3000, 40).tolist(), list(range(3000))):
        want = np.zeros(3000, dtype=np.uint8)
        for s in seeds:
            want[walk(F.parent, s)[0]] = 1
        assert du.marks_of(F.parent, F.depth, seeds).tolist() == want.tolist()


def test_map_partials_and_pruned_against_plain_loops():
    rng = np.random.default_rng(3)
    F = du.random_forest(1000, 3)
    p = du.payload(1000, index=rng.integers(0, 50, 1000), n_bad=(rng.random(1000) < 0.4), status=rng.integers(0, 3, 1000) // 2)
    assert p.digest.reshape(-1, 8)[:, 0].tolist() == [(8 * i * 2654435761) & 0xFFFFFFFF for i in range(1000)]
    assert len(set(p.digest.tolist())) == 8000 and (p.prev == ~p.digest).all()
    G = du.SimpleNamespace(n=1000, parent=F.parent, **vars(p))
    marks = du.marks_of(F.parent, F.depth, rng.integers(0, 1000, 30).tolist())
    assert 0 < marks.sum() < 1000
    kept, new = du.map_of(marks)
    want, j = [], 0
    for m in marks.tolist():
        want.append(j if m else POOL_NONE)
        j += m
    assert new.tolist() == want and kept == j
    assert du.partials_of(marks).tolist() == [int(marks[k:k + 256].sum()) for k in range(0, 1000, 256)]
    # K12e's statement: the partials' exclusive scan plus the rank inside the 256
    scan = np.concatenate([[0], np.cumsum(du.partials_of(marks))[:-1]])
    for i in np.flatnonzero(marks).tolist():
        assert new[i] == scan[i // 256] + int(marks[i - i % 256:i].sum())
    r = du.pruned(G, marks)
    keep = [i for i in range(1000) if marks[i]]
    assert r.kept == len(keep) and r.index.tolist() == [int(p.index[i]) for i in keep]
    assert r.parent.tolist() == [want[F.parent[i]] if F.parent[i] < 1000 else int(F.parent[i]) for i in keep]
    assert POOL_NONE not in [want[F.parent[i]] for i in keep if F.parent[i] < 1000]  # closed under parent
    assert r.digest.reshape(-1, 8).tolist() == [p.digest[8 * i:8 * i + 8].tolist() for i in keep]
    assert r.status.tolist() == [int(p.status[i]) for i in keep] and r.n_flagged == sum(1 for i in keep if p.status[i])
    best = None
    for j, i in enumerate(keep):  # K10e's rule in words: the greatest index among the sound, the first of them on a tie
        if p.n_bad[i] == 0 and (best is None or p.index[i] > p.index[keep[best]]):
            best = j
    assert r.best == (int(p.index[keep[best]]) << 32 | (~best & 0xFFFFFFFF))
    assert du.best_of([3, 9, 9], [0, 1, 1]) == 3 << 32 | 0xFFFFFFFF and du.best_of([3], [2]) == 0
    assert du.best_of([4, 9, 9, 2], [0, 0, 0, 0]) == 9 << 32 | 0xFFFFFFFE


def test_marks_by_index():
    pattern = np.random.default_rng(4).integers(0, 2, 777)
    M = du.marks_by_index(pattern)
    assert (M.parent == POOL_ROOT).all() and (M.min_index, M.flags) == (1, du.KEEP_BY_INDEX)
    assert ((M.index >= M.min_index) == (pattern != 0)).all() and M.index[pattern != 0].tolist() == (np.flatnonzero(pattern) + 1).tolist()
    assert du.rounds(1) == 0 and du.rounds(2) == 1 and du.rounds(1 << 20) == 20 and du.rounds((1 << 19) + 1) == 20
    assert [du.rows(n) for n in (0, 1, 2, 3, 4, 5, 64, 65, 1 << 20)] == [0, 0, 0, 1, 1, 2, 5, 6, 19]


# ---- the hooks ----
def test_the_hooks_are_in_the_test_library_only():
    shipped, test = _lib.load(), _lib.load(test_hooks=True)
    for name in HOOKS:
        assert name not in _lib.EXPORTS
        assert not hasattr(shipped, name) and getattr(test, name)
        assert name.encode() not in open(_lib.LIB_PATH, "rb").read() and name.encode() in open(_lib.TEST_LIB_PATH, "rb").read()
    assert ctypes.sizeof(du.PruneIO) == 23 * 8 and ctypes.sizeof(du.LiftIO) == 13 * 8  # the hooks' static_asserts


FAKE = ctypes.c_void_p(8)  # a context that is never dereferenced: every case fails before it would be


def last(L):
    return (L.pow_last_error() or b"").decode()


def test_prune_hook_einval_without_a_gpu():
    L = _lib.load(test_hooks=True)
    prune, _ = du.hooks(L)
    assert prune(FAKE, (1 << 20) + 1, None) == _lib.POW_EINVAL and "too many nodes" in last(L)
    assert prune(FAKE, 1 << 40, None) == _lib.POW_EINVAL and "too many nodes" in last(L)
    assert prune(FAKE, 4, None) == _lib.POW_EINVAL and "null" in last(L)
    assert prune(None, 4, ctypes.byref(du.PruneIO())) == _lib.POW_EINVAL and "null" in last(L)
    assert prune(None, 0, None) == _lib.POW_EINVAL
    M = du.marks_by_index([1, 0, 1, 1])

    def call(F=M, n=4, **kw):
        F = du.SimpleNamespace(**{**vars(F), **{k: v for k, v in kw.items() if k == "parent"}})
        rc, o = du.run_prune(L, FAKE, F, **{k: v for k, v in kw.items() if k != "parent"})
        assert (o.marks == 0xEE).all() and o.kept[0] == du.POISON and (o.map == du.POISON).all()  # nothing is written
        return rc, last(L)

    for flags in (4, 8, 0x80000001):
        rc, msg = call(flags=flags, fin=2, tips=[9])
        assert rc == _lib.POW_EINVAL and "unknown flags" in msg
    rc, msg = call(fin=2, tips=[9])
    assert rc == _lib.POW_EINVAL and "fin 2" in msg
    rc, msg = call(tips=np.zeros((1 << 16) + 1, dtype=np.uint32))
    assert rc == _lib.POW_EINVAL and "too many tips" in msg
    for tip in (4, POOL_NONE, POOL_ROOT):
        rc, msg = call(tips=[0, 3, tip])
        assert rc == _lib.POW_EINVAL and f"tip 2 (node {tip}) past the forest's 4" in msg
    for bad in (4, 5, POOL_NONE - 1):
        rc, msg = call(parent=np.array([POOL_ROOT, 0, bad, POOL_NONE], dtype=np.uint32))
        assert rc == _lib.POW_EINVAL and f"parent {bad} of node 2" in msg
    io = du.PruneIO()
    io.n_tips = 1
    assert prune(FAKE, 4, ctypes.byref(io)) == _lib.POW_EINVAL and "null tips" in last(L)
    io.n_tips = 0
    assert prune(FAKE, 4, ctypes.byref(io)) == _lib.POW_EINVAL and "null" in last(L) and "tips" not in last(L)
    assert prune(FAKE, 0, ctypes.byref(io)) == 0  # nothing to do, and nothing touched


def test_lift_hook_einval_without_a_gpu():
    L = _lib.load(test_hooks=True)
    _, lift = du.hooks(L)
    assert lift(FAKE, (1 << 20) + 1, None) == _lib.POW_EINVAL and "too many nodes" in last(L)
    assert lift(FAKE, 4, None) == _lib.POW_EINVAL and "null" in last(L)
    assert lift(None, 4, ctypes.byref(du.LiftIO())) == _lib.POW_EINVAL and "null" in last(L)
    C = du.shuffled_list(6, 1, covered=3)
    fine = np.array([0, 5, 2], dtype=np.uint32)
    past = np.array([0, 6, 2], dtype=np.uint32)

    def call(mode=du.ANCESTORS, in0=fine, in1=fine, parent=C.parent, **kw):
        rc, o = du.run_lift(L, FAKE, parent, C.depth, mode, in0, in1, **kw)
        outs = o.out if isinstance(o.out, tuple) else (o.out,)
        assert all((x == du.POISON).all() for x in outs) and o.launches == du.POISON  # nothing is written
        return rc, last(L)

    for capacity in (5, 0, (1 << 20) + 1):
        rc, msg = call(capacity=capacity, covered=7, mode=3)
        assert rc == _lib.POW_EINVAL and f"capacity {capacity} outside 6..2^20" in msg
    rc, msg = call(covered=7, mode=3)
    assert rc == _lib.POW_EINVAL and "covered 7 past the forest's 6" in msg
    rc, msg = call(mode=3)
    assert rc == _lib.POW_EINVAL and "unknown mode 3" in msg
    rc, msg = call(mode=du.CHAIN, in0=None, in1=None, k=7, tip=9)
    assert rc == _lib.POW_EINVAL and "too many queries (7 > 6)" in msg
    rc, msg = call(k=(1 << 20) + 1, in0=past)
    assert rc == _lib.POW_EINVAL and "too many queries" in msg
    for mode, a, b in ((du.ANCESTORS, past, fine), (du.FORKS, past, fine), (du.FORKS, fine, past)):
        rc, msg = call(mode=mode, in0=a, in1=b)
        assert rc == _lib.POW_EINVAL and "query 1 names a node past the forest's 6" in msg
    for tip in (6, POOL_NONE, POOL_ROOT):
        rc, msg = call(mode=du.CHAIN, in0=None, in1=None, k=3, tip=tip)
        assert rc == _lib.POW_EINVAL and f"tip (node {tip}) past the forest's 6" in msg
    bad = C.parent.copy()
    bad[4] = 6
    rc, msg = call(parent=bad)
    assert rc == _lib.POW_EINVAL and "parent 6 of node 4" in msg
    for covered in (1, 2, 4, 5):  # the list's first three heights are the positions 0..2, the rest lie behind
        closed = all(p < covered or p >= 6 for p in C.parent[:covered].tolist())
        rc, msg = call(covered=covered, parent=C.parent if not closed else bad)
        assert rc == _lib.POW_EINVAL and ("not closed under parent" in msg) == (not closed)
    io = du.LiftIO()
    io.k, io.capacity = 1, 4
    assert lift(FAKE, 4, ctypes.byref(io)) == _lib.POW_EINVAL and "null" in last(L)
    io.capacity = 0
    assert lift(FAKE, 0, ctypes.byref(io)) == _lib.POW_EINVAL  # k = 1 queries on nothing
    io.k = 0
    assert lift(FAKE, 0, ctypes.byref(io)) == 0  # nothing to do


# ---- the hooks run the library's own launch sequences ----
SEQUENCE_LAUNCHERS = ("pow_launch_pool_round(", "pow_launch_pool_finish(", "pow_launch_pool_prune_seed(",
                      "pow_launch_pool_prune_round(", "pow_launch_pool_prune_count(", "pow_launch_pool_prune_scan(",
                      "pow_launch_pool_prune_gather(", "pow_launch_pool_prune_remap(", "pow_launch_pool_lift_row(",
                      "pow_launch_pool_lift_small(")
SEQUENCES = ("pow_queue_pool_rank", "pow_queue_pool_mark", "pow_queue_pool_compact", "pow_queue_pool_lift")


def function_bodies(text):
    """(name, body) of every function defined at file level in `text` (comments
    and literals already blanked): a definition starts in column 0 and ends at
    the next closing brace in column 0, as everywhere under csrc/."""
    out = []
    for m in re.finditer(r"^[A-Za-z_][^\n;{}()]*?\b(\w+)\s*\([^;{}]*\)\s*\{", text, flags=re.M):
        out.append((m.group(1), text[m.end():text.index("\n}", m.end())]))
    return out


def test_each_shared_launch_sequence_is_stated_once():
    """K10d/K10e, K12a to K12f and K13a/K13b are queued by pow_queue_pool_*
    (csrc/pow_api.cpp) and by nothing else in the host sources: the calls
    and the hooks of the deep tests run the same statements, so a test that
    reaches 2^20 nodes holds the shipped sequence."""
    from test_build import CSRC, POOL_API, _strip_comments_and_strings

    users = {name: [] for name in SEQUENCE_LAUNCHERS}
    for f in sorted(os.listdir(CSRC)):
        if not f.endswith((".cpp", ".h")):
            continue
        text = _strip_comments_and_strings(open(os.path.join(CSRC, f)).read())
        bodies = function_bodies(text)
        for name in SEQUENCE_LAUNCHERS:
            inside = sum(body.count(name) for _, body in bodies)
            # outside a body: nothing but the wrapper's declaration in pow_ctx.h
            assert text.count(name) - inside == (1 if f == "pow_ctx.h" else 0), (f, name)
            users[name] += [(f, fn) for fn, body in bodies if name in body]
    for name, where in users.items():
        assert len(where) == 1, (name, where)
        assert where[0][0] == POOL_API and where[0][1] in SEQUENCES, (name, where)
    assert {fn for where in users.values() for _, fn in where} == set(SEQUENCES)
    hooks = _strip_comments_and_strings(open(os.path.join(CSRC, "pow_hooks.cpp")).read())
    for name in SEQUENCE_LAUNCHERS:
        assert name not in hooks, name
    for name in SEQUENCES:
        assert f"{name}(ctx->stream, " in hooks, name
    # the instrument sees a seeded copy: a launcher called from a second function
    seeded = "int copy(pow_ctx* ctx) {\n  return (int)pow_launch_pool_round(ctx->stream, D, 0);\n}\n"
    assert [fn for fn, body in function_bodies(seeded) if "pow_launch_pool_round(" in body] == ["copy"]
