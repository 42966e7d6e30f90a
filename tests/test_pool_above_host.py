"""pow_pool_tips, pow_pool_subtrees and pow_pool_drop on the host (CPU only):
the Python mirror (block.BlockPool.tips, .subtrees and .drop, the GPU tests'
yardstick) against the header's definitions restated in numpy over
parent / depth / n_bad / index; the export list, the prototypes and the
null-pool check of the C calls; and the kernels' own membership test in
tests/pool_above_plan_unit.cpp, a process of its own under sanitizers."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from mpi_blockchain_amd import _lib
from mpi_blockchain_amd.block import POOL_NONE, POOL_ROOT, BlockPool, index_blocks, prune_structs

import pool_util as pu
from test_abi import header_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pow_pool_tips", "pow_pool_subtrees", "pow_pool_drop")


def arrays(mirror):
    return tuple(np.array(a, dtype=np.uint32) for a in (mirror.parent, mirror.depth, mirror.n_bad, mirror.index))


def brute_tips(parent, n_bad, sound_only):
    """Block i is a tip when no block j has parent[j] == i."""
    n = len(parent)
    named = np.zeros(n, dtype=bool)
    named[parent[parent < n]] = True
    keep = ~named & ((n_bad == 0) | (not sound_only))
    return np.flatnonzero(keep).tolist()


def brute_members(parent, root):
    """Per block: does `root` lie on the walk from it along parent?  n rounds of stepping every walk at once."""
    n = len(parent)
    at = np.arange(n, dtype=np.int64)
    hit = np.zeros(n, dtype=bool)
    for _ in range(n + 1):
        live = at < n
        if not live.any():
            break
        hit |= live & (at == root)
        at = np.where(live, parent[np.minimum(at, n - 1)], at)
    return hit


def brute_subtrees(parent, depth, n_bad, index, roots):
    n = len(parent)
    size, height, best, best_index, on = [], [], [], [], np.zeros(n, dtype=np.uint8)
    for r in roots:
        m = brute_members(parent, r)
        on |= m.astype(np.uint8)
        size.append(int(m.sum()))
        height.append(int((depth[m].astype(np.int64) - int(depth[r])).max()))
        sound = np.flatnonzero(m & (n_bad == 0))
        if len(sound):
            top = int(index[sound].max())
            pick = int(sound[index[sound] == top][0])  # the lowest position of the greatest index
            best.append(pick), best_index.append(top)
        else:
            best.append(POOL_NONE), best_index.append(0)
    return size, height, best, best_index, on.tolist()


def check_mirror(mirror, roots):
    parent, depth, n_bad, index = arrays(mirror)
    got = mirror.subtrees(roots)
    assert tuple(got) == brute_subtrees(parent, depth, n_bad, index, roots), roots
    return got


def check_drop(blocks, difficulty, roots):
    """The mirror's drop against the contract: index_blocks on the survivors, then on the survivors plus an add."""
    mirror = BlockPool(difficulty)
    mirror.add(blocks)
    on = mirror.subtrees(roots)[4]
    new = mirror.drop(roots)
    kept, want = 0, []
    for m in on:
        want.append(POOL_NONE if m else kept)
        kept += not m
    assert new == want
    survivors = prune_structs(blocks, new)
    assert len(mirror) == len(survivors) == kept
    assert mirror.results() == index_blocks(survivors, difficulty) if survivors else len(mirror) == 0
    dropped = [b for b, j in zip(blocks, new) if j == POOL_NONE]
    mirror.add(dropped)  # the dropped blocks come back
    assert mirror.results() == index_blocks(survivors + dropped, difficulty)
    return new


@pytest.mark.parametrize("order", ["mined", "shuffled"])
def test_mirror_on_the_tree(order):
    blocks = pu.tree()
    if order == "shuffled":
        blocks, _ = pu.shuffled(blocks, 5)
    mirror = BlockPool(pu.D)
    mirror.add(blocks[:13]), mirror.add(blocks[13:])
    parent, depth, n_bad, index = arrays(mirror)
    for sound_only in (False, True):
        assert mirror.tips(sound_only) == brute_tips(parent, n_bad, sound_only)
    assert len(mirror.tips()) == 6  # the branch, the race, its two losers, the top and the second root's chain
    check_mirror(mirror, list(range(40)))
    check_mirror(mirror, [3, 3, 0, 17, 39, 0])  # duplicates and nested roots
    roots = [i for i in range(40) if mirror.parent[i] == POOL_ROOT]
    size = mirror.subtrees(roots)[0]
    assert sorted(size) == [8, 32] and mirror.subtrees(roots)[4] == [1] * 40
    for r in range(40):
        check_drop(blocks, pu.D, [r])
    check_drop(blocks, pu.D, roots)  # everything goes
    check_drop(blocks, pu.D, [])     # nothing goes
    check_drop(blocks, pu.D, mirror.tips())


@pytest.mark.parametrize("seed,difficulty", pu.FUZZ)
def test_mirror_on_the_fuzz_pools(seed, difficulty):
    blocks = pu.random_pool(seed)
    mirror = BlockPool(difficulty)
    mirror.add(blocks[:len(blocks) // 3]), mirror.add(blocks[len(blocks) // 3:])
    parent, depth, n_bad, index = arrays(mirror)
    rng = np.random.default_rng(seed)
    n = len(mirror)
    for sound_only in (False, True):
        tips = mirror.tips(sound_only)
        assert tips == brute_tips(parent, n_bad, sound_only) and tips
    roots = rng.integers(0, n, 12).tolist()
    size = check_mirror(mirror, roots + roots[:2])[0]
    assert max(size) > 1
    big = int(np.argmax([mirror.subtrees([r])[0][0] for r in range(min(n, 60))]))
    check_drop(blocks, difficulty, [big] + roots[:3])


def test_mirror_refuses_a_position_past_the_pool():
    mirror = BlockPool(0)
    mirror.add(pu.flat_chain(3, 0, seed=2))
    for call in (lambda: mirror.subtrees([3]), lambda: mirror.drop([0, 3]), lambda: mirror.subtrees([-1])):
        with pytest.raises(ValueError):
            call()
    assert len(mirror) == 3 and mirror.tips() == [2] and mirror.subtrees([]) == ([], [], [], [], [0, 0, 0])
    assert BlockPool(0).tips() == []


def test_the_names_are_exported_from_both_libraries_and_the_hook_from_one():
    for name in NAMES:
        assert name in _lib.EXPORTS and name in header_functions()
    for test in (False, True):
        L = _lib.load(test)
        for name in NAMES:
            assert getattr(L, name) is not None
    assert hasattr(_lib.load(True), "pow_test_pool_above") and not hasattr(_lib.load(False), "pow_test_pool_above")
    header = open(os.path.join(ROOT, "include", "pow_gpu.h")).read()
    assert "enum { POW_TIPS_SOUND_ONLY = 1 };" in header and "#define POW_POOL_MAX_ROOTS 64" in header
    assert (_lib.POW_TIPS_SOUND_ONLY, _lib.POOL_MAX_ROOTS) == (1, 64)


def test_a_null_pool_is_einval_without_a_gpu():
    """The first check of each call, in front of every later fault, with nothing written."""
    for test in (False, True):
        L = _lib.load(test)
        buf = (ctypes.c_uint32 * 4)(*[0xA5A5A5A5] * 4)
        n = ctypes.c_size_t(77)
        info = _lib.PoolInfo(*[0xA5A5A5A5] * 9)
        assert L.pow_pool_tips(None, 0xFF, None, 4, None) == _lib.POW_EINVAL
        assert b"null pool" in L.pow_last_error()
        assert L.pow_pool_tips(None, 0, buf, 4, ctypes.byref(n)) == _lib.POW_EINVAL
        assert L.pow_pool_subtrees(None, None, 65, buf, buf, buf, buf, None, ctypes.byref(n)) == _lib.POW_EINVAL
        assert b"null pool" in L.pow_last_error()
        assert L.pow_pool_drop(None, None, 65, buf, ctypes.byref(info)) == _lib.POW_EINVAL
        assert b"null pool" in L.pow_last_error()
        assert list(buf) == [0xA5A5A5A5] * 4 and n.value == 77 and info.size == 0xA5A5A5A5


def test_above_plan_unit_under_sanitizers(tmp_path):
    """tests/pool_above_plan_unit.cpp compiles pow_above_dev.h and pow_lift_dev.h with a host compiler, links
    pow_host.cpp alone and runs as a process of its own under ASan + UBSan: nothing is loaded into Python."""
    csrc = os.path.join(ROOT, "mpi_blockchain_amd", "csrc")
    exe = str(tmp_path / "pool_above_plan_unit")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                    os.path.join(ROOT, "tests", "pool_above_plan_unit.cpp"), os.path.join(csrc, "pow_host.cpp"), "-o", exe],
                   check=True, cwd=str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert " checks, 0 failed" in r.stdout, r.stdout
    assert int(r.stdout.split(" checks, 0 failed")[0].split()[-1]) > 2_000_000
