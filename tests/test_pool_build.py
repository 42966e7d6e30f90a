"""Codegen and source guards for K10, the kernels of pow_index_blocks
(csrc/pow_pool.hip; CPU only: hipcc cross-compiles gfx950).  Metadata and
source checks only."""
import os
import re
import subprocess
import tempfile

import pytest

from mpi_blockchain_amd import _lib

from test_build import CSRC, POOL_API, ROOT, api_function, null_stream_calls, pool_function, timed_section_helpers

SRC = "pow_pool.hip"
SHARED = "pow_audit_dev.h"
KERNELS = {"audit": "_Z21pow_pool_audit_kernel", "insert": "_Z22pow_pool_insert_kernel",
           "join": "_Z20pow_pool_join_kernel", "round": "_Z21pow_pool_round_kernel",
           "finish": "_Z22pow_pool_finish_kernel"}


@pytest.fixture(scope="module")
def isa():
    from mpi_blockchain_amd.build import hipcc

    with tempfile.TemporaryDirectory() as td:
        subprocess.run([hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-mcode-object-version=5",
                        "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-c",
                        os.path.join(CSRC, SRC), "-o", os.path.join(td, "p.o"),
                        "-save-temps=obj"], check=True, cwd=td, capture_output=True)
        s = [f for f in os.listdir(td) if f.endswith("gfx950.s")]
        assert s
        return open(os.path.join(td, s[0])).read()


def kernel_metadata(isa: str, prefix: str) -> dict:
    for blk in isa.split("  - .agpr_count")[1:]:
        nm = re.search(r"\.name:\s+(\S+)", blk)
        if nm and nm.group(1).startswith(prefix):
            return {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", blk, flags=re.M)}
    raise AssertionError(prefix)


@pytest.mark.parametrize("which", sorted(KERNELS))
def test_pool_kernels_have_no_scratch_and_no_spills(isa, which):
    md = kernel_metadata(isa, KERNELS[which])
    assert md["private_segment_fixed_size"] == 0, md
    assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md
    assert md["wavefront_size"] == 64, md
    m = re.search(rf"^({KERNELS[which]}\w*):[^\n]*\n(.*?)s_endpgm", isa, flags=re.S | re.M)
    assert m and not re.search(r"^\s+scratch_", m.group(2), flags=re.M)


def test_pool_audit_kernel_fits_beside_k1(isa):
    """K10a keeps K3's budget: 64 VGPRs, and the LDS of its 64 blocks alone (no halo)."""
    md = kernel_metadata(isa, KERNELS["audit"])
    assert md["vgpr_count"] <= 64, md
    assert md["group_segment_fixed_size"] == 64 * 552, md
    assert md["max_flat_workgroup_size"] == 64, md
    for which in ("insert", "join", "round", "finish"):
        assert kernel_metadata(isa, KERNELS[which])["group_segment_fixed_size"] == 0, which


def test_pool_audit_kernel_loads_its_tile_in_16_byte_vectors(isa):
    m = re.search(rf"^({KERNELS['audit']}\w*):[^\n]*\n(.*?)s_endpgm", isa, flags=re.S | re.M)
    assert m
    body = m.group(2)
    assert "global_load_dwordx4" in body and re.search(r"ds_write_b128|ds_store_b128", body)
    assert "global_store_dwordx4" in body  # the digest and the parsed name, 16 bytes at a time


def test_pool_kernels_are_in_both_libraries():
    from mpi_blockchain_amd import build

    for test in (False, True):
        assert os.path.join(CSRC, SRC) in build.sources(test=test)
    assert SRC not in build.TEST_ONLY and SHARED in build.HEADERS
    for path in (_lib.LIB_PATH, _lib.TEST_LIB_PATH):
        lib = open(path, "rb").read()
        for k in KERNELS.values():
            assert k.encode() in lib, (path, k)


def test_no_null_stream_in_pool_sources():
    found = {}
    for f in (SRC, SHARED, POOL_API, "pow_ctx.h", "pow_hooks.cpp"):
        hits = null_stream_calls(open(os.path.join(CSRC, f)).read())
        if hits:
            found[f] = hits
    assert not found, found
    kernel = open(os.path.join(CSRC, SRC)).read()
    assert kernel.count("hipLaunchKernelGGL(") == 5 and "<<<" not in kernel and "hipGraph" not in kernel


def test_index_blocks_has_one_bounded_wait_after_the_tiles():
    """The tile walk is pow_verify_chain's; behind it one timed section holds
    the reset, K10b to K10e and the copies down, with one bounded wait.  K10d
    and K10e are the one statement of the rank, pow_queue_pool_rank."""
    body, h = pool_function("pow_index_blocks"), timed_section_helpers()
    rank = pool_function("pow_queue_pool_rank", "hipError_t")
    assert not null_stream_calls(body + rank)
    assert "hipStreamSynchronize" not in rank and "hipGraph" not in rank and "hipEvent" not in rank
    assert body.count("verify_tiles(") == 1 and "pow_launch_pool_audit(ctx->stream" in body
    after = body[body.index("[](const VerifyTile&) {}))"):]
    assert after.count("timed_begin(") == 1 and after.count("timed_end(") == 1
    assert "timed_begin(" not in body[:body.index("verify_tiles(")]
    assert body.count("timed_begin(") == 1 and body.count("timed_end(") == 1
    assert "stream_wait" not in body and "hipStreamSynchronize" not in body and "hipGraph" not in body
    assert h["timed_end"].count("stream_wait_for(") == 1
    order = [after.index(s) for s in ("timed_begin(", "hipMemsetAsync(D.table", "pow_launch_pool_insert(",
                                      "pow_launch_pool_join(", "pow_queue_pool_rank(ctx->stream, D, plan.rounds)",
                                      "hipEventRecord(ctx->ev1", "hipMemcpyAsync(", "timed_end(")]
    assert order == sorted(order)
    # the rank: `rounds` rounds, then the finish on the buffers the last round wrote
    order = [rank.index(s) for s in ("for (uint32_t r = 0; r < rounds; ++r)", "pow_launch_pool_round(stream, D, r)",
                                     "pow_launch_pool_finish(stream, D, rounds & 1u)")]
    assert order == sorted(order)
    assert re.findall(r"\bfor \(([^;]*);", rank) == ["uint32_t r = 0"]
    assert "for (" not in body and "while" not in body + rank
    # the table is reset on every call, over all of its slots
    assert "hipMemsetAsync(D.table, 0xFF, (size_t)D.slots * sizeof(uint32_t), ctx->stream)" in after
    # only what the caller asked for comes down
    for out in ("status", "parent", "depth", "n_bad"):
        assert re.search(rf"if \({out}\) HIP_OK\(hipMemcpyAsync\({out}, ", after), out
    assert "padded_message" not in body and "for (size_t i" not in body  # no per-block host work
    # the argument checks come first, in the stated order
    checks = [body.index(s) for s in ("diff_bits > 256", "n > POW_POOL_MAX_BLOCKS", "!ctx ||", "ctx->stats")]
    assert checks == sorted(checks)


def test_the_shared_header_still_holds_the_one_compression():
    text = open(os.path.join(CSRC, SRC)).read()
    assert f'#include "{SHARED}"' in text and "compress(" not in text
    assert "hash_block(" in text and "own_flags(" in text and "load_tile(" in text
    shared = open(os.path.join(CSRC, SHARED)).read()
    assert shared.count("compress(h, w)") == 1 and "__forceinline__ uint32_t audit_block(" in shared
    assert "__forceinline__ void hash_block(" in shared


def test_insert_never_spins():
    """Every probe loop is a for loop bounded by the table's size; the slot
    word is touched by atomics only in K10b, and nothing fences."""
    code = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, SRC)).read())
    assert "while" not in code and "__threadfence" not in code and "volatile" not in code
    assert code.count("for (uint32_t probe = 0; probe <= mask; ++probe)") == 2
    insert = code[code.index("void pow_pool_insert_kernel"):code.index("void pow_pool_join_kernel")]
    assert re.findall(r"\batomic\w+", insert) == ["atomicCAS", "atomicMin", "atomicOr"]
    assert "table[" not in insert.replace("&table[slot]", "")  # no plain access to a slot


def test_switch_and_rank_hook_only_in_the_test_library():
    shipped = open(_lib.LIB_PATH, "rb").read()
    test = open(_lib.TEST_LIB_PATH, "rb").read()
    for s in (b"POW_POOL_SLOTS_LOG2", b"pow_test_pool_rank", b"pow_test_pool_prune", b"pow_test_pool_lift"):
        assert s not in shipped and s in test, s
    for f in os.listdir(CSRC):
        p = os.path.join(CSRC, f)
        if os.path.isfile(p) and f != "pow_hooks.cpp":
            assert 'getenv("POW_POOL' not in open(p).read(), f


def test_warmup_does_not_launch_the_kernels():
    assert "pow_launch_pool" not in api_function("pow_warmup")
