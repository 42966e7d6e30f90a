"""examples/pool_above.c builds against the shipped library and runs: what it
prints is the mirror's (block.BlockPool) over the structs it dumped, and the
launches are the header's closed forms."""
import ctypes
import os
import re
import subprocess

import pytest

from mpi_blockchain_amd._lib import PKG, Block
from mpi_blockchain_amd.block import POOL_NONE, BlockPool

from test_pool_lift_gpu import rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_example(tmp_path):
    exe, dump = str(tmp_path / "pool_above"), str(tmp_path / "pool.bin")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "pool_above.c"), "-L", PKG, "-lpow_gpu",
                    f"-Wl,-rpath,{PKG}", "-o", exe], check=True)
    heights = 6
    p = subprocess.run([exe, str(heights), "9", dump], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    raw = open(dump, "rb").read()
    n = 1 + 3 * heights
    assert len(raw) == n * ctypes.sizeof(Block)
    blocks = list((Block * n).from_buffer_copy(raw))
    mirror = BlockPool(9)
    mirror.add(blocks)
    assert mirror.ok
    tips = mirror.tips(True)
    assert tips == [heights, 2 * heights, 3 * heights]
    assert f"3 sound tips: {' '.join(map(str, tips))}; 5 launches\n" in p.stdout
    roots = [1, 1 + heights, 1 + 2 * heights]
    size, height, best, best_index, _ = mirror.subtrees(roots)
    assert size == [3 * heights, 2 * heights, heights]
    for r in range(3):
        assert (f"rival {r}'s first block {roots[r]}: {size[r]} blocks on it, {height[r]} confirmations, "
                f"best tip above it {best[r]} at index {best_index[r]}\n") in p.stdout
    assert best == [3 * heights] * 3  # the third rival's tip stands highest, and on all three
    assert f"subtrees: {rows(n) + 1} launches\n" in p.stdout  # the table from nothing, then K14d
    new = mirror.drop([roots[1]])
    gone = sum(1 for j in new if j == POOL_NONE)
    assert gone == 2 * heights and len(mirror) == n - gone
    m = re.search(r"^dropped block (\d+) and what stood on it: (\d+) blocks gone, size (\d+) flagged (\d+) best (-?\d+) "
                  r"index (\d+) capacity (\d+); (\d+) launches$", p.stdout, flags=re.M)
    # the table is up to date from the subtrees' call: K14d, K12c, K12d, then K12e, K12f, K10b
    assert [int(x) for x in m.groups()] == [roots[1], gone, len(mirror), 0, mirror.best, mirror.index[mirror.best], 64, 6]
    left = mirror.tips()
    assert left == [heights] and f"1 tips left: {heights}\n" in p.stdout
    assert f"pool of {n} blocks at difficulty 9: {len(mirror)} left, sound 1" in p.stdout
