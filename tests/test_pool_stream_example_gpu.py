"""examples/pool_stream.c builds against the shipped library and runs: every
line it prints per add is the mirror's (block.BlockPool) over the pool it
dumped, and the chain it prints is the mirror's best chain."""
import ctypes
import os
import re
import subprocess

import pytest

from mpi_blockchain_amd._lib import PKG, Block
from mpi_blockchain_amd.block import POOL_ROOT, BlockPool

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_example(tmp_path):
    exe, dump = str(tmp_path / "pool_stream"), str(tmp_path / "pool.bin")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "pool_stream.c"), "-L", PKG, "-lpow_gpu",
                    f"-Wl,-rpath,{PKG}", "-o", exe], check=True)
    p = subprocess.run([exe, "6", "9", dump], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    raw = open(dump, "rb").read()
    n = 1 + 3 * 6
    assert len(raw) == n * ctypes.sizeof(Block)
    blocks = (Block * n).from_buffer_copy(raw)
    adds = re.findall(r"^add (\d+): size (\d+) flagged (\d+) best (-?\d+) index (\d+) adopted (\d+) reranked (\d+) "
                      r"rehashed \d+ capacity \d+ slots \d+; (\d+) launches$", p.stdout, flags=re.M)
    assert len(adds) == n
    mirror, reranks = BlockPool(9), 0
    for i, line in enumerate(adds):
        mirror.add([blocks[i]])
        best = -1 if mirror.best is None else mirror.best
        rr = int(mirror.adopted > 0)
        reranks += rr
        assert [int(x) for x in line] == [i, i + 1, mirror.n_flagged, best, 0 if best < 0 else blocks[best].index,
                                          mirror.adopted, rr, 4 + rr * (3 + i.bit_length())], (i, line)
    assert mirror.ok and mirror.depth[mirror.best] == 7 and reranks > 0
    assert f"pool of {n} blocks fed one by one: {reranks} adds ranked it again; equal to one pow_index_blocks call" in p.stdout
    printed = re.findall(r"^block (\d+) at (\d+) owner (\d+) nonce (\S{9}) hash ([0-9a-f]{64})$", p.stdout, flags=re.M)
    walk = [mirror.best]
    while mirror.parent[walk[-1]] != POOL_ROOT:
        walk.append(mirror.parent[walk[-1]])
    assert printed == [(str(blocks[at].index), str(at), str(blocks[at].node_owner_number), blocks[at].nonce.decode(),
                        blocks[at].block_hash.decode()) for at in walk]
    assert "best chain of 7 blocks at difficulty 9" in p.stdout
