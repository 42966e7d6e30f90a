"""examples/pool_fork.c builds against the shipped library and runs: every
reorg it prints is the mirror's (block.BlockPool) over the structs it dumped,
fed in the same order, and the launches are the plan's."""
import ctypes
import os
import re
import subprocess

import pytest

from mpi_blockchain_amd._lib import PKG, Block
from mpi_blockchain_amd.block import POOL_NONE, BlockPool

from test_pool_lift_gpu import lift_launches, rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_example(tmp_path):
    exe, dump = str(tmp_path / "pool_fork"), str(tmp_path / "pool.bin")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "pool_fork.c"), "-L", PKG, "-lpow_gpu",
                    f"-Wl,-rpath,{PKG}", "-o", exe], check=True)
    heights = 6
    p = subprocess.run([exe, str(heights), "9", dump], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    raw = open(dump, "rb").read()
    n = 1 + 3 * heights
    assert len(raw) == n * ctypes.sizeof(Block)
    blocks = (Block * n).from_buffer_copy(raw)
    printed = re.findall(r"^add (\d+): best (\d+) -> (\d+): fork point (-?\d+), (\d+) back, (\d+) forward; (\d+) launches\n"
                         r"  roll back((?: \d+)*); (\d+) launches\n  apply((?: \d+)*); (\d+) launches$", p.stdout, flags=re.M)
    mirror, best, want, covered = BlockPool(9), None, [], 0
    for i in range(n):
        mirror.add([blocks[i]])
        assert mirror.ok and mirror.adopted == 0  # a sound pool without orphans: the table is only ever extended
        old, best = best, mirror.best
        if old is None or best == old or mirror.parent[best] == old:
            continue
        at, back_old, back_new = mirror.fork_point(old, best)
        assert at != POOL_NONE and back_old >= 1 and back_new == back_old + 1  # the new chain is one block longer
        launches = lift_launches(covered, i + 1, covered == 0) + 1
        covered = i + 1
        want.append((str(i), str(old), str(best), str(at), str(back_old), str(back_new), str(launches),
                     "".join(f" {b}" for b in mirror.chain(old, back_old)), "1",
                     "".join(f" {b}" for b in mirror.chain(best, back_new)[::-1]), "1"))
    assert printed == want and len(want) == 4
    assert any(int(w[4]) > 1 for w in want)  # a reorg that rolls back more than one block
    last = mirror.best
    assert mirror.index[last] == 2 * 2 + heights  # the third rival's tip: two forks, each two blocks up
    assert (f"pool of {n} blocks fed one by one at difficulty 9: {len(want)} reorgs; best {last} at index "
            f"{mirror.index[last]}; table of {rows(covered)} rows, {4 * 64 * 5} bytes") in p.stdout
