"""pow_pool on the host (CPU only): the incremental Python mirror
(block.BlockPool, the GPU tests' yardstick) against block.index_blocks over
the blocks added so far, after every add; the export list and the argument
checks in their stated order; and the host plan in
tests/pool_live_plan_unit.cpp, a process of its own under sanitizers."""
import ctypes
import os
import random
import subprocess

import pytest

from mpi_blockchain_amd import _lib
from mpi_blockchain_amd.block import POOL_NONE, BlockPool, index_blocks

import pool_util as pu
import verify_util as vu
from test_abi import header_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pow_pool_open", "pow_pool_close", "pow_pool_add", "pow_pool_get_info", "pow_pool_read", "pow_pool_find")


def batches_of(blocks, sizes):
    """`blocks` cut into batches of the given sizes, the last size repeated."""
    out, at, k = [], 0, 0
    while at < len(blocks):
        m = sizes[min(k, len(sizes) - 1)]
        out.append(blocks[at:at + m])
        at, k = at + m, k + 1
    return out


def feed_and_compare(blocks, batches, difficulty):
    """The mirror after every add against index_blocks over everything added;
    returns the adds' adopted counts."""
    mirror, so_far, adopted = BlockPool(difficulty), [], []
    for batch in batches:
        before = index_blocks(so_far, difficulty)[1]
        ok = mirror.add(batch)
        so_far += batch
        status, parent, depth, n_bad, best = index_blocks(so_far, difficulty)
        assert (mirror.status, mirror.parent, mirror.depth, mirror.n_bad, mirror.best) == \
            (status, parent, depth, n_bad, best)
        assert ok == mirror.ok == (not any(status)) and mirror.n_flagged == sum(1 for s in status if s)
        assert len(mirror) == len(so_far)
        # adopted: the earlier orphans that have a parent now
        assert mirror.adopted == sum(1 for i, p in enumerate(before) if p == POOL_NONE and parent[i] != POOL_NONE)
        adopted.append(mirror.adopted)
    assert so_far == list(blocks)
    return adopted


@pytest.fixture(scope="module")
def tree():
    return pu.tree(seed=3)


@pytest.mark.parametrize("order", ["mined", "reversed", "shuffled"])
@pytest.mark.parametrize("sizes", [(1,), (2,), (3,), (7,), (27,), (39, 1), (1, 39)])
def test_mirror_after_every_add_of_the_tree(tree, order, sizes):
    blocks = {"mined": list(tree), "reversed": tree[::-1], "shuffled": pu.shuffled(tree, 5)[0]}[order]
    adopted = feed_and_compare(blocks, batches_of(blocks, sizes), pu.D)
    if order == "mined":
        assert not any(adopted)  # every parent in front of its children
    if order == "reversed" and sizes == (1,):
        # a block that is somebody's parent adopts as it comes: all but the tips
        _, parent, *_ = index_blocks(blocks, pu.D)
        assert [a > 0 for a in adopted] == [k in parent for k in range(40)]


@pytest.mark.parametrize("seed,difficulty", pu.FUZZ[:4])
def test_mirror_after_every_add_of_a_fuzz_pool(seed, difficulty):
    pool = pu.random_pool(seed)
    rng = random.Random(seed)
    sizes = tuple(rng.randint(1, 130) for _ in range(len(pool)))
    adopted = feed_and_compare(pool, batches_of(pool, sizes), difficulty)
    assert adopted[0] == 0 and any(adopted)  # a shuffled pool: parents come late


def test_mirror_find_is_a_dict_lookup(tree):
    blocks = [pu.copy_block(b) for b in pu.shuffled(tree, 6)[0]]
    vu.flip_hash_digit(blocks, 9)  # no name: its stored text finds nothing
    twin = pu.copy_block(blocks[4])
    twin.index += 256              # not hashed: blocks[4]'s digest at a higher position
    blocks.append(twin)
    mirror = BlockPool(pu.D)
    for batch in batches_of(blocks, (7,)):
        mirror.add(batch)
    status = index_blocks(blocks, pu.D)[0]
    names = {}
    for i, b in enumerate(blocks):
        if not status[i] & 1:
            names.setdefault(pu.name_of(b), i)
    for i, b in enumerate(blocks):
        assert mirror.find(pu.name_of(b)) == names.get(pu.name_of(b), POOL_NONE)
    assert mirror.find(pu.name_of(blocks[9])) == POOL_NONE and mirror.find(pu.name_of(twin)) == 4
    assert mirror.find(b"0" * 64) == POOL_NONE and mirror.find(pu.name_of(blocks[0])[:63]) == POOL_NONE


def test_the_names_are_exported():
    assert set(NAMES) <= set(_lib.EXPORTS) and set(_lib.EXPORTS) == header_functions()
    for lib in (_lib.load(), _lib.load(test_hooks=True)):
        for name in NAMES:
            assert getattr(lib, name)
    assert ctypes.sizeof(_lib.PoolInfo) == 36
    header = open(os.path.join(ROOT, "include", "pow_gpu.h")).read()
    fields = header[header.index("typedef struct pow_pool_info {"):header.index("} pow_pool_info;")]
    assert [n for n, _ in _lib.PoolInfo._fields_] == \
        [n for line in fields.split("\n")[1:] for n in line.split(";")[0].replace("uint32_t", "").replace(",", " ").split()]


def test_einval_in_the_stated_order():
    """Each case has every LATER fault too, and the message names the first.
    Nothing is written, and no context is touched (there is none)."""
    L = _lib.load()
    err = lambda: (L.pow_last_error() or b"").decode()  # noqa: E731
    out = ctypes.c_void_p(77)
    # pow_pool_open: diff_bits, reserve, the null pointers
    for d in (257, 1 << 31):
        assert L.pow_pool_open(None, d, (1 << 20) + 1, None) == _lib.POW_EINVAL and "diff_bits" in err()
    assert L.pow_pool_open(None, 256, (1 << 20) + 1, None) == _lib.POW_EINVAL and "reserve" in err()
    assert L.pow_pool_open(None, 0, 1 << 20, ctypes.byref(out)) == _lib.POW_EINVAL and "null" in err()
    fake = ctypes.c_void_p(8)  # never dereferenced: the null out fails first
    assert L.pow_pool_open(fake, 0, 0, None) == _lib.POW_EINVAL and "null" in err()
    assert out.value == 77
    # the calls on a pool: a null pool first
    info = _lib.PoolInfo(*[0xA5A5A5A5] * 9)
    words = (ctypes.c_uint32 * 4)(*[0xA5A5A5A5] * 4)
    blocks = (_lib.Block * 1)()
    assert L.pow_pool_add(None, None, 1 << 40, ctypes.byref(info)) == _lib.POW_EINVAL and "null pool" in err()
    assert L.pow_pool_add(None, blocks, 1, ctypes.byref(info)) == _lib.POW_EINVAL and "null pool" in err()
    assert L.pow_pool_get_info(None, ctypes.byref(info)) == _lib.POW_EINVAL and "null" in err()
    assert L.pow_pool_read(None, 1 << 40, 1 << 40, None, words, words, words) == _lib.POW_EINVAL and "null pool" in err()
    assert L.pow_pool_find(None, None, 1 << 40, words) == _lib.POW_EINVAL and "null pool" in err()
    L.pow_pool_close(None)  # nothing to do
    assert list(words) == [0xA5A5A5A5] * 4 and info.size == info.slots == 0xA5A5A5A5


def test_plan_under_sanitizers(tmp_path):
    """tests/pool_live_plan_unit.cpp links pow_host.cpp alone and runs as a
    process of its own under ASan + UBSan: nothing is loaded into Python."""
    csrc = os.path.join(ROOT, "mpi_blockchain_amd", "csrc")
    exe = str(tmp_path / "pool_live_plan_unit")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                    os.path.join(ROOT, "tests", "pool_live_plan_unit.cpp"), os.path.join(csrc, "pow_host.cpp"),
                    "-o", exe], check=True, cwd=str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert " checks, 0 failed" in r.stdout, r.stdout
    assert int(r.stdout.split(" checks, 0 failed")[0].split()[-1]) > 20_000  # the sweeps ran
