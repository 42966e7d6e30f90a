"""examples/index_blocks.c builds against the shipped library and runs: the
chain it prints is the best chain of the mirror (block.index_blocks and
block.chain_from) over the pool it dumped."""
import ctypes
import os
import re
import subprocess

import pytest

from mpi_blockchain_amd._lib import PKG, Block
from mpi_blockchain_amd.block import POOL_ROOT, chain_from, index_blocks, verify_chain

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_example(tmp_path):
    exe, dump = str(tmp_path / "index_blocks"), str(tmp_path / "pool.bin")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "index_blocks.c"), "-L", PKG, "-lpow_gpu",
                    f"-Wl,-rpath,{PKG}", "-o", exe], check=True)
    p = subprocess.run([exe, "6", "9", dump], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    raw = open(dump, "rb").read()
    n = 1 + 3 * 6
    assert len(raw) == n * ctypes.sizeof(Block)
    pool = (Block * n).from_buffer_copy(raw)
    status, parent, depth, n_bad, best = index_blocks(pool, 9)
    assert not any(status) and parent.count(POOL_ROOT) == 1 and depth[best] == 7
    assert f"pool of {n} blocks: 1 root, {n - len(set(parent) - {POOL_ROOT})} tips, no block flagged; 9 launches" in p.stdout
    printed = re.findall(r"^block (\d+) at (\d+) owner (\d+) nonce (\S{9}) hash ([0-9a-f]{64})$", p.stdout, flags=re.M)
    chain = chain_from(pool, parent, best)
    walk = [best]
    while parent[walk[-1]] != POOL_ROOT:
        walk.append(parent[walk[-1]])
    assert printed == [(str(b.index), str(at), str(b.node_owner_number), b.nonce.decode(), b.block_hash.decode())
                       for b, at in zip(chain, walk)]
    assert not any(verify_chain(chain, 9)) and "best chain of 7 blocks at difficulty 9: valid" in p.stdout
