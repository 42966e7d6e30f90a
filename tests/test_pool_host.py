"""pow_index_blocks on the host (CPU only): the Python mirror
(block.index_blocks, the GPU tests' yardstick) against block.verify_chain on
the chains block.chain_from extracts; the argument checks in their stated
order; the export list; and the host plan in tests/pool_plan_unit.cpp, a
process of its own under sanitizers."""
import ctypes
import os
import subprocess

import pytest

from mpi_blockchain_amd import _lib
from mpi_blockchain_amd.block import (POOL_NONE, POOL_ROOT, V_HASH, V_INDEX, V_LINK, V_WORK, chain_from, index_blocks,
                                      verify_chain)

import pool_util as pu
import verify_util as vu
from test_abi import header_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tree():
    return pu.tree(seed=3)


def test_the_name_is_exported():
    assert "pow_index_blocks" in _lib.EXPORTS and set(_lib.EXPORTS) == header_functions()
    assert _lib.load().pow_index_blocks and _lib.load(test_hooks=True).pow_index_blocks
    assert (_lib.POOL_MAX_BLOCKS, _lib.POOL_ROOT, _lib.POOL_NONE) == (1 << 20, 0xFFFFFFFF, 0xFFFFFFFE)
    header = open(os.path.join(ROOT, "include", "pow_gpu.h")).read()
    for text in ("#define POW_POOL_MAX_BLOCKS (1u << 20)", "#define POW_POOL_ROOT 0xFFFFFFFFu",
                 "#define POW_POOL_NONE 0xFFFFFFFEu"):
        assert text in header
    for hook in ("pow_test_pool_rank", "pow_test_pool_prune", "pow_test_pool_lift"):
        assert not hasattr(_lib.load(), hook) and getattr(_lib.load(test_hooks=True), hook) and hook not in _lib.EXPORTS


def test_plan_under_sanitizers(tmp_path):
    """tests/pool_plan_unit.cpp links pow_host.cpp alone and runs as a process
    of its own under ASan + UBSan: nothing is loaded into Python."""
    csrc = os.path.join(ROOT, "mpi_blockchain_amd", "csrc")
    exe = str(tmp_path / "pool_plan_unit")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                    os.path.join(ROOT, "tests", "pool_plan_unit.cpp"), os.path.join(csrc, "pow_host.cpp"), "-o", exe],
                   check=True, cwd=str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert " checks, 0 failed" in r.stdout, r.stdout
    assert int(r.stdout.split(" checks, 0 failed")[0].split()[-1]) > 25_000  # the sweep ran


def test_einval_in_the_stated_order():
    """diff_bits, n, the null pointers: each case has every LATER fault too,
    and the message names the first.  Nothing is written."""
    L = _lib.load()
    out = (ctypes.c_uint32 * 4)(*[0xA5A5A5A5] * 4)
    best = ctypes.c_size_t(77)
    pool = (_lib.Block * 1)()

    def call(ctx, blocks, n, d):
        rc = L.pow_index_blocks(ctx, blocks, n, d, None, out, out, out, ctypes.byref(best))
        return rc, (L.pow_last_error() or b"").decode()

    for d in (257, 1 << 31):
        rc, msg = call(None, None, (1 << 20) + 1, d)
        assert rc == _lib.POW_EINVAL and "diff_bits" in msg, msg
    for n in ((1 << 20) + 1, 1 << 40):
        rc, msg = call(None, None, n, 256)
        assert rc == _lib.POW_EINVAL and "too large" in msg, msg
    fake = ctypes.c_void_p(8)  # never dereferenced: the null pool fails first
    for ctx, blocks, n in ((None, pool, 1), (None, None, 0), (fake, None, 1), (None, pool, 1 << 20)):
        rc, msg = call(ctx, blocks, n, 0)
        assert rc == _lib.POW_EINVAL and "null" in msg, msg
    assert list(out) == [0xA5A5A5A5] * 4 and best.value == 77


def test_mirror_on_a_valid_tree(tree):
    pool, perm = pu.shuffled(tree, 11)
    status, parent, depth, n_bad, best = index_blocks(pool, pu.D)
    assert status == [0] * 40 and n_bad == [0] * 40
    assert sorted(parent.count(r) for r in (POOL_ROOT, POOL_NONE)) == [0, 2]
    where = {p: k for k, p in enumerate(perm)}  # position in `tree` -> position in the pool
    # the trunk: root + 12, then the branch of 4 on its tip: the deepest block, and the highest index
    assert depth[where[0]] == 1 and depth[where[12]] == 13
    assert max(depth) == 17 and depth.index(17) == best and pool[best].index == max(b.index for b in pool)
    for i in range(40):
        p = parent[i]
        if p < 40:
            assert depth[i] == depth[p] + 1 and pu.name_of(pool[p]) == pool[i].previous_block_hash
    assert all(pu.sound_tips(pool, pu.D))


@pytest.mark.parametrize("what", ["hash", "work", "removed", "index", "nonce"])
def test_mirror_against_verify_chain_on_extracted_chains(tree, what):
    """A tip has n_bad == 0 exactly when its chain_from chain has an all-zero
    verify_chain status and ends at a root."""
    blocks = [pu.copy_block(b) for b in tree]
    d = pu.D
    if what == "hash":      # the trunk's fifth block, where the branch forks: no name, its children are orphans
        vu.flip_hash_digit(blocks, 5)
    elif what == "work":    # what both roots still have, above what some block mined at 4 or 5 has
        d = min(vu.leading_zero_bits(blocks[0]), vu.leading_zero_bits(blocks[32]))
    elif what == "removed":
        del blocks[5]
    elif what == "index":
        blocks[5].index = 99  # not hashed beyond its low byte: 99 != 6 there too, so the hash goes with it
    elif what == "nonce":
        vu.flip_nonce(blocks, 20)
    pool, _ = pu.shuffled(blocks, 12)
    status, parent, depth, n_bad, best = index_blocks(pool, d)
    sound = pu.sound_tips(pool, d)
    assert [b == 0 for b in n_bad] == sound
    assert any(sound) and not all(sound)
    assert best is not None and sound[best]
    assert pool[best].index == max(b.index for b, ok in zip(pool, sound) if ok)
    flagged = [s for s in status if s]
    if what in ("hash", "removed"):
        assert flagged.count(V_LINK) == 2  # the next trunk block and the branch's first
        assert (V_HASH in flagged) == (what == "hash")
    if what == "work":
        assert set(flagged) == {V_WORK}
    # n_bad counts the flagged blocks of the walk
    for i in range(len(pool)):
        walk, j = [], i
        while j < len(pool):
            walk.append(j)
            j = parent[j]
        assert depth[i] == len(walk) and n_bad[i] == sum(1 for k in walk if status[k])
        assert (j == POOL_NONE) == bool(status[walk[-1]] & V_LINK)


# ---- what the inputs of tests/test_pool_edges_gpu.py hold, from the mirror alone ----
@pytest.mark.parametrize("case", sorted(pu.TIE_CASES))
def test_mirror_on_the_tie_pools(case):
    pool, best = pu.tie_pool(case)
    index, flagged, _ = pu.TIE_CASES[case]
    status, parent, depth, n_bad, got = index_blocks(pool, 0)
    assert len(pool) == 600 and got == best
    assert status == [V_HASH if k in flagged else 0 for k in range(600)] and n_bad == [s and 1 for s in status]
    assert parent == [POOL_ROOT] * 600 and [b.index for b in pool] == [index.get(k, 9) for k in range(600)]
    assert len({pu.name_of(b) for b in pool}) == 600  # no twins: the position alone breaks a tie


def test_mirror_on_the_twin_storm():
    for low_index, other_index in ((1, 257), (257, 1)):
        pool, children = pu.twin_storm(low_index, other_index)
        status, parent, depth, n_bad, best = index_blocks(pool, 0)
        assert len(pool) == 804 and len({pu.name_of(b) for b in pool}) == 5 and pu.twins_in(pool, status) == 799
        assert [parent[k] for k in children] == [3] * 100 and parent.count(POOL_ROOT) == 704
        assert {status[k] for k in children} == {0 if low_index == 1 else V_INDEX}
        status, parent, depth, n_bad, best = index_blocks(pool[::-1], 0)
        assert [parent[803 - k] for k in children] == [1] * 100
        assert {status[803 - k] for k in children} == {0 if other_index == 1 else V_INDEX}


def test_mirror_on_the_name_sweep():
    pool, name = pu.name_sweep()
    assert len(pool) == 16321 and len(name) == 64 and set(name) == set(b"0123456789abcdef")
    status, parent, depth, n_bad, best = index_blocks(pool, 0)
    assert parent == [POOL_ROOT] * 2 + [POOL_NONE] * 16319 and status == [0] * 2 + [V_LINK] * 16319
    assert pool[1].previous_block_hash == b"" and best == 1 and pool[1].index == 2


def test_fuzz_pools_hold_every_case():
    """Each pool has a sound tip and a flagged block; over the 24, every flag,
    a twin and an orphan occur."""
    pools_with = {V_HASH: 0, V_WORK: 0, V_LINK: 0, V_INDEX: 0, "twin": 0, "orphan": 0}
    assert len(pu.FUZZ) == 24 and [d for _, d in pu.FUZZ] == [0, 1, 3] * 8
    for seed, d in pu.FUZZ:
        pool = pu.random_pool(seed)
        status, parent, depth, n_bad, best = index_blocks(pool, d)
        assert 190 <= len(pool) <= 715 and 0 in n_bad and any(status) and best is not None, (seed, d)
        for f in (V_HASH, V_WORK, V_LINK, V_INDEX):
            pools_with[f] += any(s & f for s in status)
        pools_with["twin"] += pu.twins_in(pool, status) > 0
        pools_with["orphan"] += POOL_NONE in parent
        # the sound tips are exactly those whose extracted chain passes verify_chain down to a root
        assert [b == 0 for b in n_bad] == pu.sound_tips(pool, d), seed
    assert all(pools_with.values()), pools_with
    assert pools_with[V_WORK] == 16  # at d = 1 and d = 3, from the blocks' own digests; none at d = 0


def test_mirror_index_rule_and_duplicates():
    c = pu.flat_chain(4, 0, seed=21)
    # a wrong index in the high bytes is not hashed: only V_INDEX, on the block and on its child
    c[2].index += 1 << 8
    status, parent, depth, n_bad, best = index_blocks(c, 0)
    assert status == [0, 0, V_INDEX, V_INDEX] and parent == [POOL_ROOT, 0, 1, 2] and n_bad == [0, 0, 1, 2] and best == 1
    # two blocks of one digest (they differ in a byte that is not hashed): the lowest position is the parent
    c = pu.flat_chain(3, 0, seed=22)
    twin = pu.copy_block(c[1])
    twin.index += 256
    for pool, par, st in (([c[0], c[1], twin, c[2]], 1, [0, 0, V_INDEX, 0]),
                          ([c[0], twin, c[1], c[2]], 1, [0, V_INDEX, 0, V_INDEX])):
        status, parent, depth, n_bad, best = index_blocks(pool, 0)
        assert parent == [POOL_ROOT, 0, 0, par] and status == st
    # index 0 over 0xFFFFFFFF passes
    c = vu.build_chain(3, 0, seed=23)
    vu.index_wrap(c, 0)
    vu.seal(c[1], 0, 5)  # the index's low byte is hashed: a new name, which its child takes up
    ctypes.memmove(ctypes.addressof(c[0]) + _lib.Block.previous_block_hash.offset,
                   ctypes.addressof(c[1]) + _lib.Block.block_hash.offset, 256)
    vu.seal(c[0], 0, 5)
    status, parent, depth, n_bad, best = index_blocks(list(c), 0)
    assert c[0].index == 0 and c[1].index == 0xFFFFFFFF and parent == [1, 2, POOL_ROOT]
    assert status == [0, V_INDEX, 0] and best == 2  # 0xFFFFFFFF over c[2].index + 1 does not pass; c[0] sits on it
    assert verify_chain(chain_from(list(c), parent, 0), 0) == status
