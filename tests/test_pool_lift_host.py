"""pow_pool_ancestors, pow_pool_fork_points and pow_pool_chain on the host (CPU
only): the Python mirror (block.BlockPool.ancestor, .fork_point and .chain,
the GPU tests' yardstick) against an independent statement; the export list
and the null-pool check of the C calls; and the host plan with the kernels'
own per-lane walks in tests/pool_lift_plan_unit.cpp, a process of its own
under sanitizers, up to the pool's limit of 2^20 blocks."""
import ctypes
import os
import random
import subprocess

import pytest

from mpi_blockchain_amd import _lib
from mpi_blockchain_amd.block import POOL_NONE, POOL_ROOT, BlockPool, chain_from

import pool_util as pu
from test_abi import header_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pow_pool_ancestors", "pow_pool_fork_points", "pow_pool_chain", "pow_pool_lift_get_info")


def walk_of(mirror: BlockPool, i: int):
    """(the blocks on the walk from i in order, the walk's end)."""
    out = []
    while i < len(mirror):
        out.append(i)
        i = mirror.parent[i]
        assert len(out) <= len(mirror)  # names are digests: no walk comes back to itself
    assert i in (POOL_ROOT, POOL_NONE)
    return out, i


def plain_ancestor(mirror, pos, steps):
    walk, end = walk_of(mirror, pos)
    return walk[steps] if steps < len(walk) else end


def plain_fork(mirror, a, b):
    """The issue's words: the first block on a's walk that also lies on b's,
    by the set of b's ancestors; the steps by the block's place in each walk."""
    wa, wb = walk_of(mirror, a)[0], walk_of(mirror, b)[0]
    on_b = set(wb)
    for x in wa:
        if x in on_b:
            return x, wa.index(x), wb.index(x)
    return POOL_NONE, len(wa), len(wb)


def fed(blocks, difficulty, cuts=(3,)):
    mirror = BlockPool(difficulty)
    at = 0
    for c in cuts:
        mirror.add(blocks[at:len(blocks) // c])
        at = len(blocks) // c
    mirror.add(blocks[at:])
    assert len(mirror) == len(blocks)
    return mirror


def check_chain(mirror, blocks, tip, max_len):
    got = mirror.chain(tip, max_len)
    walk = walk_of(mirror, tip)[0]
    assert got == (walk if max_len is None else walk[:max_len])
    assert len(walk) == mirror.depth[tip]
    if max_len is None:  # the structs chain_from extracts along the same parents
        want = chain_from(blocks, mirror.parent, tip)
        assert len(want) == len(got)
        assert bytes(want) == b"".join(bytes(blocks[j]) for j in got)


@pytest.mark.parametrize("order", ["mined", "shuffled"])
def test_mirror_on_the_tree_every_query(order):
    blocks = pu.tree()
    if order == "shuffled":
        blocks, _ = pu.shuffled(blocks, 5)
    mirror = fed(blocks, pu.D, cuts=(4, 2))
    n, asked = len(mirror), 0
    for a in range(n):
        for b in range(n):
            assert mirror.fork_point(a, b) == plain_fork(mirror, a, b), (a, b)
            asked += 1
        for steps in list(range(mirror.depth[a] + 3)) + [0xFFFFFFFF]:
            assert mirror.ancestor(a, steps) == plain_ancestor(mirror, a, steps), (a, steps)
        for max_len in (None, 0, 1, 5, mirror.depth[a], mirror.depth[a] + 1):
            check_chain(mirror, blocks, a, max_len)
    assert asked == 1600
    # two roots in the tree: blocks on different roots share nothing
    roots = [i for i in range(n) if mirror.parent[i] == POOL_ROOT]
    assert len(roots) == 2
    ends = {r: [i for i in range(n) if walk_of(mirror, i)[0][-1] == r] for r in roots}
    a, b = ends[roots[0]][-1], ends[roots[1]][-1]
    assert mirror.fork_point(a, b) == (POOL_NONE, mirror.depth[a], mirror.depth[b])


@pytest.mark.parametrize("seed,difficulty", pu.FUZZ)
def test_mirror_on_the_fuzz_pools(seed, difficulty):
    blocks = pu.random_pool(seed)
    mirror = fed(blocks, difficulty)
    rng = random.Random(seed)
    n = len(mirror)
    seen_none = 0
    for _ in range(2000):
        a, b = rng.randrange(n), rng.randrange(n)
        got = mirror.fork_point(a, b)
        assert got == plain_fork(mirror, a, b), (a, b)
        seen_none += got[0] == POOL_NONE
        steps = rng.choice((rng.randrange(mirror.depth[a] + 3), mirror.depth[a] - 1, mirror.depth[a], 0xFFFFFFFF))
        assert mirror.ancestor(a, steps) == plain_ancestor(mirror, a, steps), (a, steps)
    assert seen_none  # several roots and orphans in every one of these pools
    for tip in rng.sample(range(n), 50):
        check_chain(mirror, blocks, tip, rng.choice((None, 3, mirror.depth[tip])))


def test_mirror_on_a_flat_chain_of_64():
    blocks = pu.flat_chain(64, 0, seed=9)
    mirror = fed(blocks, 0)
    assert mirror.depth[63] == 64
    assert mirror.ancestor(63, 63) == 0 and mirror.ancestor(63, 64) == POOL_ROOT == mirror.ancestor(63, 0xFFFFFFFF)
    for a in range(64):
        for b in range(64):
            assert mirror.fork_point(a, b) == (min(a, b), a - min(a, b), b - min(a, b)) == plain_fork(mirror, a, b)
        for steps in range(67):
            assert mirror.ancestor(a, steps) == (a - steps if steps <= a else POOL_ROOT)
        assert mirror.chain(a) == list(range(a, -1, -1))
        check_chain(mirror, blocks, a, None)


def test_mirror_refuses_a_position_past_the_pool():
    mirror = fed(pu.flat_chain(3, 0, seed=2), 0)
    for call in (lambda: mirror.ancestor(3, 0), lambda: mirror.fork_point(3, 0), lambda: mirror.fork_point(0, 3),
                 lambda: mirror.chain(3), lambda: mirror.ancestor(-1, 0), lambda: mirror.chain(POOL_NONE, 2)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError):
        BlockPool(0).chain(0)


def test_the_names_are_exported_from_both_libraries():
    for name in NAMES:
        assert name in _lib.EXPORTS and name in header_functions()
    for test in (False, True):
        L = _lib.load(test)
        for name in NAMES:
            assert getattr(L, name) is not None


def test_a_null_pool_is_einval_without_a_gpu():
    for test in (False, True):
        L = _lib.load(test)
        buf = (ctypes.c_uint32 * 4)(*[0xA5A5A5A5] * 4)
        n = ctypes.c_size_t(77)
        assert L.pow_pool_ancestors(None, buf, buf, 4, buf) == _lib.POW_EINVAL
        assert b"null pool" in L.pow_last_error()
        assert L.pow_pool_fork_points(None, buf, buf, 4, buf, buf, buf) == _lib.POW_EINVAL
        assert b"null pool" in L.pow_last_error()
        assert L.pow_pool_chain(None, 0, 4, buf, ctypes.byref(n)) == _lib.POW_EINVAL
        assert b"null pool" in L.pow_last_error()
        assert L.pow_pool_lift_get_info(None, ctypes.byref(_lib.PoolLiftInfo())) == _lib.POW_EINVAL
        assert list(buf) == [0xA5A5A5A5] * 4 and n.value == 77
    assert ctypes.sizeof(_lib.PoolLiftInfo) == 32


def test_lift_plan_unit_under_sanitizers(tmp_path):
    """tests/pool_lift_plan_unit.cpp links pow_host.cpp alone and runs as a
    process of its own under ASan + UBSan: nothing is loaded into Python."""
    csrc = os.path.join(ROOT, "mpi_blockchain_amd", "csrc")
    exe = str(tmp_path / "pool_lift_plan_unit")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                    os.path.join(ROOT, "tests", "pool_lift_plan_unit.cpp"), os.path.join(csrc, "pow_host.cpp"), "-o", exe],
                   check=True, cwd=str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert " checks, 0 failed" in r.stdout, r.stdout
    assert int(r.stdout.split(" checks, 0 failed")[0].split()[-1]) > 80_000_000  # the forests and the lists of 2^20 ran
