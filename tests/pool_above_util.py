"""The test library's hook that runs K14 on a forest of the caller's making
(pow_test_pool_above, csrc/pow_hooks.cpp), and numpy statements of what it must
give: the tips, the subtrees' records and marks, and a drop's map and survivors.
Everything here is numpy over parent, depth, index and n_bad: no block is
hashed.  tests/test_pool_above_deep_gpu.py runs the kernels on pool_deep_util's
forests of up to 2^20 nodes."""
import ctypes
from types import SimpleNamespace

import numpy as np

from mpi_blockchain_amd.block import POOL_NONE

from pool_deep_util import POISON, U32, _p, _u32, u8p, u32p

TIPS, SUBTREES, DROP = 0, 1, 2
SOUND_ONLY, MAX_ROOTS = 1, 64
u64p = ctypes.POINTER(ctypes.c_uint64)


class AboveIO(ctypes.Structure):
    """pow_test_above_io (csrc/pow_hooks.cpp)."""
    _fields_ = [("parent", u32p), ("depth", u32p), ("index", u32p), ("n_bad", u32p), ("roots", u32p),
                ("k", ctypes.c_size_t), ("mode", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("fin", ctypes.c_uint32),
                ("pad", ctypes.c_uint32), ("marks", u8p), ("total", u32p), ("list", u32p), ("size", u32p),
                ("height", u32p), ("best", u64p), ("map", u32p), ("parent_out", u32p), ("depth_out", u32p)]


assert ctypes.sizeof(AboveIO) == 17 * 8


def run_above(L, ctx, parent, depth, index, n_bad, mode, roots=(), flags=0, fin=0):
    """pow_test_pool_above; every output is poisoned first.  Returns (rc, the
    outputs): marks, total, and by mode the list cut to the total, the records
    of the k roots, the map and the survivors' parent and depth cut to the total."""
    parent, depth, index, n_bad, roots = _u32(parent), _u32(depth), _u32(index), _u32(n_bad), _u32(list(roots))
    n, k = len(parent), len(roots)
    o = SimpleNamespace(marks=np.full(n, 0xEE, dtype=np.uint8), total=np.full(1, POISON, dtype=U32),
                        list=np.full(n, POISON, dtype=U32), size=np.full(k + 1, POISON, dtype=U32),
                        height=np.full(k + 1, POISON, dtype=U32), best=np.full(k + 1, POISON, dtype=np.uint64),
                        map=np.full(n, POISON, dtype=U32), parent=np.full(n, POISON, dtype=U32),
                        depth=np.full(n, POISON, dtype=U32))
    io = AboveIO(_p(parent), _p(depth), _p(index), _p(n_bad), _p(roots), k, mode, flags, fin, 0, _p(o.marks, u8p),
                 _p(o.total), _p(o.list), _p(o.size), _p(o.height), o.best.ctypes.data_as(u64p), _p(o.map), _p(o.parent),
                 _p(o.depth))
    L.pow_test_pool_above.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(AboveIO)]
    L.pow_test_pool_above.restype = ctypes.c_int
    rc = L.pow_test_pool_above(ctx, n, ctypes.byref(io))
    if rc == 0 and n:
        t = o.total = int(o.total[0])
        assert o.size[k] == o.height[k] == POISON and o.best[k] == POISON  # nothing behind the k records
        o.size, o.height, o.best = o.size[:k], o.height[:k], o.best[:k]
        o.list = o.list[:t] if mode == TIPS else o.list
        if mode == DROP:
            for name in ("parent", "depth"):
                whole = getattr(o, name)
                assert (whole[t:] == POISON).all(), name  # nothing behind the survivors
                setattr(o, name, whole[:t])
    return rc, o


# ---- numpy statements ----
def tips_of(parent, n_bad, sound_only=False):
    """Block i is a tip when no block j has parent[j] == i (and, sound_only, n_bad[i] == 0): the marks."""
    n = len(parent)
    named = np.zeros(n, dtype=bool)
    named[parent[parent < n]] = True
    return (~named & ((n_bad == 0) | (not sound_only))).astype(np.uint8)


def members_of(parent, root):
    """Per node: does `root` lie on the walk from it?  By doubling: hit_k says
    it for the first 2^k nodes of the walk, jump_k is the node 2^k steps along."""
    n = len(parent)
    hit = np.arange(n) == root
    jump = parent.astype(np.int64)
    while True:
        live = jump < n
        if not live.any():
            return hit
        at = np.where(live, jump, 0)
        hit = hit | (live & hit[at])
        jump = np.where(live, jump[at], jump)


def key_of(index, n_bad, members):
    """K10e's key over `members`: the greatest index << 32 | ~position among n_bad == 0; 0 = none."""
    pos = np.flatnonzero(members & (n_bad == 0)).astype(np.uint64)
    if not len(pos):
        return 0
    return int(((index[pos.astype(np.int64)].astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - pos)).max())


def subtrees_of(parent, depth, index, n_bad, roots):
    """(size, height, key per root, the marks of the union)."""
    on = np.zeros(len(parent), dtype=np.uint8)
    size, height, best = [], [], []
    for r in roots:
        m = members_of(parent, int(r))
        on |= m.astype(np.uint8)
        size.append(int(m.sum()))
        height.append(int(depth[m].max()) - int(depth[r]))
        best.append(key_of(index, n_bad, m))
    return size, height, best, on


def dropped(parent, depth, keep):
    """(map, the survivors' parent, their depth) of a drop that keeps the marks `keep`, closed under parent."""
    n = len(parent)
    keep = keep.astype(bool)
    new = np.where(keep, np.cumsum(keep) - 1, POOL_NONE).astype(U32)
    par = parent[keep]
    inner = par < n
    return new, np.where(inner, new[np.where(inner, par, 0)], par).astype(U32), depth[keep]
