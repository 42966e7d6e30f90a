"""Synthetic forests of up to 2^20 nodes with closed-form answers, and the test
library's two hooks that run K12 and K13 on them (pow_test_pool_prune and
pow_test_pool_lift, csrc/pow_hooks.cpp).  Everything here is numpy: no block
is hashed, K12 and K13 read parent, depth, index, n_bad, status and the marks
and nothing else.  tests/test_pool_deep_host.py holds the generators and the
references against plain walks; tests/test_pool_deep_gpu.py runs the kernels."""
import ctypes
from types import SimpleNamespace

import numpy as np

from mpi_blockchain_amd.block import POOL_NONE, POOL_ROOT

U32 = np.uint32
KEEP_BY_INDEX, KEEP_SOUND_ONLY = 1, 2
MAX_BLOCKS, MAX_TIPS, LIFT_SMALL = 1 << 20, 1 << 16, 256
POISON = 0xEEEEEEEE  # what the lift hook fills the table with, and what the wrappers fill every output with


def rounds(n: int) -> int:
    """pow_pool_rounds: ceil(log2 n), 0 for n <= 1."""
    return (n - 1).bit_length() if n > 1 else 0


def rows(n: int) -> int:
    """pow_pool_lift_rows."""
    return max(rounds(n) - 1, 0)


# ---- generators ----
def shuffled_list(n: int, seed: int, end: int = POOL_ROOT, covered: int = 0):
    """One list of n nodes whose node at height h is order[h - 1]; its last
    parent is `end`.  covered: the first `covered` heights take the positions
    below `covered` and the rest those behind, each shuffled among themselves,
    so the positions below `covered` are closed under parent."""
    rng = np.random.default_rng(seed)
    order = np.concatenate([rng.permutation(covered), covered + rng.permutation(n - covered)]).astype(U32)
    parent = np.empty(n, dtype=U32)
    parent[order[0]] = end
    parent[order[1:]] = order[:-1]
    depth = np.empty(n, dtype=U32)
    depth[order] = np.arange(1, n + 1, dtype=U32)
    return SimpleNamespace(n=n, parent=parent, depth=depth, order=order, end=end)


def list_ancestor(L, pos, steps):
    """The node `steps` steps under pos on a shuffled_list, or its end: read off order."""
    pos, steps = np.asarray(pos, dtype=np.int64), np.asarray(steps, dtype=np.int64)
    h = L.depth[pos].astype(np.int64)
    return np.where(steps < h, L.order[np.maximum(h - 1 - steps, 0)], L.end).astype(U32)


def list_row(L, j: int):
    """Row j of the table of a shuffled_list: order[h - 1 - 2^j], or the end."""
    row = np.full(L.n, L.end, dtype=U32)
    if (1 << j) < L.n:
        row[L.order[1 << j:]] = L.order[:-(1 << j)]
    return row


def list_chain(L, tip: int, k: int):
    """(the first k nodes of the walk from tip, the walk's length capped at k)."""
    h = int(L.depth[tip])
    return L.order[:h][::-1][:k], min(h, k)


def two_arms(trunk: int, arm_a: int, arm_b: int, seed: int):
    """Two lists that share a trunk, positions shuffled.  line_a[h - 1] and
    line_b[h - 1] are the nodes at height h on either line (the first `trunk`
    are the same); side: 0 on the trunk, 1 on arm A, 2 on arm B."""
    n = trunk + arm_a + arm_b
    perm = np.random.default_rng(seed).permutation(n).astype(U32)
    line_a, b_nodes = perm[:trunk + arm_a], perm[trunk + arm_a:]
    line_b = np.concatenate([perm[:trunk], b_nodes])
    parent = np.empty(n, dtype=U32)
    parent[line_a[0]] = POOL_ROOT
    parent[line_a[1:]] = line_a[:-1]
    parent[b_nodes[:1]] = perm[trunk - 1]
    parent[b_nodes[1:]] = b_nodes[:-1]
    depth = np.empty(n, dtype=U32)
    depth[line_a] = np.arange(1, trunk + arm_a + 1, dtype=U32)
    depth[b_nodes] = np.arange(trunk + 1, trunk + arm_b + 1, dtype=U32)
    side = np.zeros(n, dtype=np.uint8)
    side[perm[trunk:trunk + arm_a]] = 1
    side[b_nodes] = 2
    return SimpleNamespace(n=n, parent=parent, depth=depth, trunk=trunk, line_a=line_a, line_b=line_b, side=side,
                           top=int(perm[trunk - 1]))


def arms_fork(T, a, b):
    """(at, back_a, back_b) on two_arms: the lower node if both are on one line, else the trunk's top."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    da, db = T.depth[a].astype(np.int64), T.depth[b].astype(np.int64)
    across = (T.side[a] != 0) & (T.side[b] != 0) & (T.side[a] != T.side[b])
    at = np.where(across, T.top, np.where(da <= db, a, b))
    to = np.where(across, T.trunk, np.minimum(da, db))
    return at.astype(U32), (da - to).astype(U32), (db - to).astype(U32)


def two_lists(n_a: int, n_b: int, seed: int):
    """Two unrelated lists, positions shuffled: A ends in POOL_ROOT, B (an orphan's walk) in POOL_NONE."""
    n = n_a + n_b
    perm = np.random.default_rng(seed).permutation(n).astype(U32)
    line_a, line_b = perm[:n_a], perm[n_a:]
    parent, depth = np.empty(n, dtype=U32), np.empty(n, dtype=U32)
    for line, end in ((line_a, POOL_ROOT), (line_b, POOL_NONE)):
        parent[line[0]] = end
        parent[line[1:]] = line[:-1]
        depth[line] = np.arange(1, len(line) + 1, dtype=U32)
    return SimpleNamespace(n=n, parent=parent, depth=depth, line_a=line_a, line_b=line_b)


def random_forest(n: int, seed: int):
    """Node k of a hidden order hangs on a random earlier one (shallow: the
    depth grows like log n), about one in 500 is another root or an orphan;
    the positions are shuffled.  hidden[k] is the position of the k-th node."""
    rng = np.random.default_rng(seed)
    par = np.zeros(n, dtype=np.int64)
    par[1:] = (rng.random(n - 1) * np.arange(1, n)).astype(np.int64)
    dice = rng.integers(0, 1000, n)
    par[dice == 0] = POOL_ROOT
    par[dice == 1] = POOL_NONE
    par[0] = POOL_ROOT
    hidden = rng.permutation(n).astype(U32)
    parent = np.empty(n, dtype=U32)
    inner = par < n
    parent[hidden] = np.where(inner, hidden[np.where(inner, par, 0)], par).astype(U32)
    return SimpleNamespace(n=n, parent=parent, depth=depths_of(parent), hidden=hidden)


def depths_of(parent):
    """The nodes on every walk, by numpy doubling (acyclic forests only)."""
    n = len(parent)
    nxt, depth = parent.astype(np.int64), np.ones(n, dtype=np.int64)
    while True:
        live = nxt < n
        if not live.any():
            return depth.astype(U32)
        at = np.where(live, nxt, 0)
        depth = depth + np.where(live, depth[at], 0)
        nxt = np.where(live, nxt[at], nxt)


def doubling_rows(parent, count: int):
    """Rows 1..count of the table by numpy doubling: row j is two jumps of level j - 1."""
    n, out, prev = len(parent), [], parent
    for _ in range(count):
        prev = np.where(prev < n, prev[np.minimum(prev, n - 1)], prev).astype(U32)
        out.append(prev)
    return out


def plain_walk(parent, pos: int):
    """(the nodes on the walk from pos in order, the walk's end): a plain Python loop."""
    out, n = [], len(parent)
    while pos < n:
        out.append(int(pos))
        pos = int(parent[pos])
    return out, pos


def plain_fork(parent, a: int, b: int):
    wa, wb = plain_walk(parent, a)[0], plain_walk(parent, b)[0]
    on_b = {x: k for k, x in enumerate(wb)}
    for k, x in enumerate(wa):
        if x in on_b:
            return x, k, on_b[x]
    return POOL_NONE, len(wa), len(wb)


# ---- K12's references ----
def payload(n: int, index=None, n_bad=None, status=None, depth=None):
    """Per-node entries that encode the node's position, so a misplaced entry
    shows: digest and prev words (8 a node), and index, depth, n_bad, status
    where the caller gives none."""
    global _WORDS
    if _WORDS is None:  # made once for the largest forest and shared: word w of all is w x 2654435761 mod 2^32
        words = (np.arange(8 * MAX_BLOCKS, dtype=np.uint64) * np.uint64(2654435761)).astype(U32)
        _WORDS = (words, ~words)
        for a in _WORDS:
            a.flags.writeable = False
    pos = np.arange(n, dtype=np.uint64)
    digest, prev = _WORDS[0][:8 * n], _WORDS[1][:8 * n]
    return SimpleNamespace(
        index=(pos + np.uint64(1)).astype(U32) if index is None else np.ascontiguousarray(index, dtype=U32),
        n_bad=np.zeros(n, dtype=U32) if n_bad is None else np.ascontiguousarray(n_bad, dtype=U32),
        status=np.zeros(n, dtype=np.uint8) if status is None else np.ascontiguousarray(status, dtype=np.uint8),
        depth=(pos * np.uint64(3) + np.uint64(7)).astype(U32) if depth is None else np.ascontiguousarray(depth, dtype=U32),
        digest=digest, prev=prev)


_WORDS = None


def marks_by_index(pattern):
    """n roots of which exactly those with pattern != 0 are seeds: index =
    position + 1 where the pattern is set, else 0, for min_index = 1 and
    POW_KEEP_BY_INDEX.  Any mark pattern, with no tree."""
    pattern = np.asarray(pattern) != 0
    n = len(pattern)
    index = np.where(pattern, np.arange(1, n + 1, dtype=np.uint64), 0).astype(U32)
    p = payload(n, index=index, status=(np.arange(n) % 251).astype(np.uint8), n_bad=(np.arange(n) % 7 == 3).astype(U32))
    return SimpleNamespace(n=n, parent=np.full(n, POOL_ROOT, dtype=U32), min_index=1, flags=KEEP_BY_INDEX, **vars(p))


def map_of(marks):
    """(kept, the map): cumsum - 1 where marked, else POOL_NONE."""
    on = np.asarray(marks) != 0
    return int(on.sum()), np.where(on, np.cumsum(on, dtype=np.int64) - 1, POOL_NONE).astype(U32)


def partials_of(marks):
    """K12c's partials: the marks of every 256 positions."""
    on = (np.asarray(marks) != 0).astype(np.int64)
    return np.add.reduceat(on, np.arange(0, len(on), 256))


def marks_of(parent, depth, seeds):
    """Every ancestor of a seed, level by level from the deepest: a node's
    mark reaches its parent, which lies one level down."""
    n = len(parent)
    on = np.zeros(n, dtype=bool)
    on[np.asarray(seeds, dtype=np.int64)] = True
    by_depth = np.argsort(depth, kind="stable")
    cuts = np.searchsorted(depth[by_depth], np.arange(1, int(depth.max()) + 2))
    for d in range(len(cuts) - 1, 0, -1):
        level = by_depth[cuts[d - 1]:cuts[d]]
        up = parent[level[on[level]]]
        on[up[up < n]] = True
    return on.astype(np.uint8)


def best_of(index, n_bad):
    """K12f's key over the survivors: the greatest index among n_bad == 0, the lowest position on a tie; 0 = none."""
    sound = np.flatnonzero(np.asarray(n_bad) == 0)
    if len(sound) == 0:
        return 0
    top = int(np.asarray(index)[sound].max())
    j = int(sound[np.asarray(index)[sound] == top][0])
    return (top << 32) | (~j & 0xFFFFFFFF)


def pruned(F, marks):
    """What a prune that keeps `marks` leaves of the forest F (parent, index,
    depth, n_bad, status, digest, prev): the marked rows in order, the parents
    by the new positions, K12f's key and flagged count."""
    kept, new = map_of(marks)
    on = np.asarray(marks) != 0
    par = F.parent[on]
    inner = par < F.n
    parent = np.where(inner, new[np.where(inner, par, 0)], par).astype(U32)
    out = SimpleNamespace(kept=kept, map=new, parent=parent, index=F.index[on], depth=F.depth[on], n_bad=F.n_bad[on],
                          status=F.status[on], digest=F.digest.reshape(-1, 8)[on].reshape(-1),
                          prev=F.prev.reshape(-1, 8)[on].reshape(-1))
    out.best, out.n_flagged = best_of(out.index, out.n_bad), int((out.status != 0).sum())
    return out


# ---- the hooks ----
u32p, u8p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint8)


class PruneIO(ctypes.Structure):
    """pow_test_prune_io (csrc/pow_hooks.cpp)."""
    _fields_ = [("parent", u32p), ("index", u32p), ("n_bad", u32p), ("status", u8p), ("depth", u32p), ("digest", u32p),
                ("prev", u32p), ("tips", u32p), ("n_tips", ctypes.c_size_t), ("min_index", ctypes.c_uint32),
                ("flags", ctypes.c_uint32), ("fin", ctypes.c_uint32), ("marks", u8p), ("kept", u32p), ("map", u32p),
                ("parent_out", u32p), ("index_out", u32p), ("depth_out", u32p), ("n_bad_out", u32p), ("status_out", u8p),
                ("digest_out", u32p), ("prev_out", u32p), ("best", ctypes.POINTER(ctypes.c_uint64)), ("n_flagged", u32p)]


class LiftIO(ctypes.Structure):
    """pow_test_lift_io (csrc/pow_hooks.cpp)."""
    _fields_ = [("parent", u32p), ("depth", u32p), ("covered", ctypes.c_uint32), ("capacity", ctypes.c_uint32),
                ("mode", ctypes.c_uint32), ("in0", u32p), ("in1", u32p), ("tip", ctypes.c_uint32), ("k", ctypes.c_size_t),
                ("out0", u32p), ("out1", u32p), ("out2", u32p), ("launches", u32p), ("table", u32p)]


ANCESTORS, FORKS, CHAIN = 0, 1, 2


def hooks(L):
    """The two exports of the test library with their argument types."""
    L.pow_test_pool_prune.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(PruneIO)]
    L.pow_test_pool_lift.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(LiftIO)]
    L.pow_test_pool_prune.restype = L.pow_test_pool_lift.restype = ctypes.c_int
    return L.pow_test_pool_prune, L.pow_test_pool_lift


def _p(a, kind=u32p):
    return a.ctypes.data_as(kind) if a is not None and len(a) else ctypes.cast(None, kind)


def _u32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=U32)


def run_prune(L, ctx, F, tips=(), min_index=0, flags=0, fin=0):
    """pow_test_pool_prune over the forest F (parent, index, n_bad, status,
    depth, digest, prev); every output is poisoned first.  Returns (rc, the
    outputs), the survivors' arrays cut to `kept` when the call passed."""
    n = len(F.parent)
    ins = [_u32(F.parent), _u32(F.index), _u32(F.n_bad), np.ascontiguousarray(F.status, dtype=np.uint8), _u32(F.depth),
           _u32(F.digest), _u32(F.prev), _u32(tips)]
    o = SimpleNamespace(marks=np.full(n, 0xEE, dtype=np.uint8), kept=np.full(1, POISON, dtype=U32),
                        map=np.full(n, POISON, dtype=U32), parent=np.full(n, POISON, dtype=U32),
                        index=np.full(n, POISON, dtype=U32), depth=np.full(n, POISON, dtype=U32),
                        n_bad=np.full(n, POISON, dtype=U32), status=np.full(n, 0xEE, dtype=np.uint8),
                        digest=np.full(8 * n, POISON, dtype=U32), prev=np.full(8 * n, POISON, dtype=U32),
                        best=np.full(1, POISON, dtype=np.uint64), n_flagged=np.full(1, POISON, dtype=U32))
    io = PruneIO(_p(ins[0]), _p(ins[1]), _p(ins[2]), _p(ins[3], u8p), _p(ins[4]), _p(ins[5]), _p(ins[6]), _p(ins[7]),
                 len(ins[7]), min_index, flags, fin, _p(o.marks, u8p), _p(o.kept), _p(o.map), _p(o.parent), _p(o.index),
                 _p(o.depth), _p(o.n_bad), _p(o.status, u8p), _p(o.digest), _p(o.prev),
                 o.best.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), _p(o.n_flagged))
    rc = hooks(L)[0](ctx, n, ctypes.byref(io))
    if rc == 0 and n:
        k = o.kept = int(o.kept[0])
        for name in ("parent", "index", "depth", "n_bad", "status"):
            whole = getattr(o, name)
            assert (whole[k:] == (0xEE if whole.dtype == np.uint8 else POISON)).all(), name  # nothing behind the survivors
            setattr(o, name, whole[:k])
        assert (o.digest[8 * k:] == POISON).all() and (o.prev[8 * k:] == POISON).all()
        o.digest, o.prev = o.digest[:8 * k], o.prev[:8 * k]
        o.best, o.n_flagged = int(o.best[0]), int(o.n_flagged[0])
    return rc, o


def run_lift(L, ctx, parent, depth, mode, in0=None, in1=None, tip=0, k=None, covered=0, capacity=None, table=False):
    """pow_test_pool_lift; every output is poisoned first.  Returns (rc, the
    outputs): out (mode FORKS: at, back_a, back_b), length (mode CHAIN),
    launches, and table (rows(n) x n) if asked for."""
    parent, depth, in0, in1 = _u32(parent), _u32(depth), _u32(in0), _u32(in1)
    n = len(parent)
    k = (len(in0) if in0 is not None else 0) if k is None else k
    outs = [np.full(k + 1, POISON, dtype=U32) for _ in range(3)]
    launches = np.full(1, POISON, dtype=U32)
    tab = np.full((rows(n), n), POISON, dtype=U32) if table else None
    io = LiftIO(_p(parent), _p(depth), covered, n if capacity is None else capacity, mode, _p(in0), _p(in1), tip, k,
                _p(outs[0]), _p(outs[1]), _p(outs[2]), _p(launches),
                tab.ctypes.data_as(u32p) if table and tab.size else ctypes.cast(None, u32p))
    rc = hooks(L)[1](ctx, n, ctypes.byref(io))
    o = SimpleNamespace(launches=int(launches[0]), table=tab, length=None)
    if mode == CHAIN:
        o.out, o.length = outs[0][:k], int(outs[0][k])
    else:
        assert all(x[k] == POISON for x in outs)  # nothing behind the answers
        o.out = outs[0][:k] if mode == ANCESTORS else tuple(x[:k] for x in outs)
    return rc, o
