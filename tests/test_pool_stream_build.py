"""Codegen and source guards for K11, the kernels of pow_pool_add and
pow_pool_find (csrc/pow_pool_live.hip; CPU only: hipcc cross-compiles gfx950).
Metadata and source checks only."""
import os
import re
import subprocess
import tempfile

import pytest

from mpi_blockchain_amd import _lib

from test_build import CSRC, POOL_API, ROOT, api_function, null_stream_calls, pool_function, timed_section_helpers
from test_pool_build import kernel_metadata

SRC = "pow_pool_live.hip"
SHARED = "pow_pool_dev.h"
KERNELS = {"insert": "_Z27pow_pool_live_insert_kernel", "join": "_Z25pow_pool_live_join_kernel",
           "round": "_Z26pow_pool_live_round_kernel", "finish": "_Z27pow_pool_live_finish_kernel",
           "strip": "_Z26pow_pool_live_strip_kernel", "find": "_Z25pow_pool_live_find_kernel"}
PROBE = "for (uint32_t probe = 0; probe <= mask; ++probe)"


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


def code() -> str:
    return re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, SRC)).read())


@pytest.mark.parametrize("which", sorted(KERNELS))
def test_live_kernels_have_no_scratch_and_no_spills(isa, which):
    md = kernel_metadata(isa, KERNELS[which])
    assert md["private_segment_fixed_size"] == 0, md
    assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md
    assert md["wavefront_size"] == 64 and md["group_segment_fixed_size"] == 0, md
    assert md["vgpr_count"] <= 64, md
    m = re.search(rf"^({KERNELS[which]}\w*):[^\n]*\n(.*?)s_endpgm", isa, flags=re.S | re.M)
    assert m and not re.search(r"^\s+scratch_", m.group(2), flags=re.M)


def test_live_kernels_are_in_both_libraries():
    from mpi_blockchain_amd import build

    for test in (False, True):
        assert os.path.join(CSRC, SRC) in build.sources(test=test)
    assert SRC not in build.TEST_ONLY and SHARED in build.HEADERS
    for path in (_lib.LIB_PATH, _lib.TEST_LIB_PATH):
        lib = open(path, "rb").read()
        for k in KERNELS.values():
            assert k.encode() in lib, (path, k)


def test_no_null_stream_in_live_sources():
    for f in (SRC, SHARED):
        assert not null_stream_calls(open(os.path.join(CSRC, f)).read()), f
    kernel = open(os.path.join(CSRC, SRC)).read()
    assert kernel.count("hipLaunchKernelGGL(") == 6 and "<<<" not in kernel and "hipGraph" not in kernel
    for name in ("pow_pool_open", "pow_pool_add", "pow_pool_read", "pow_pool_find", "pool_alloc", "pool_grow",
                 "pool_retire"):
        assert not null_stream_calls(pool_function(name)), name


def test_the_helpers_have_one_copy():
    """unhex4 and same_digest are defined in pow_pool_dev.h and nowhere else."""
    for name in ("unhex4", "same_digest"):
        definition = re.compile(rf"^__device__[^\n;=#/]*\b{name}\s*\([^;{{}}]*\)\s*\{{", flags=re.M)
        found = {f: len(definition.findall(open(os.path.join(CSRC, f)).read()))
                 for f in os.listdir(CSRC) if os.path.isfile(os.path.join(CSRC, f))}
        assert {f: n for f, n in found.items() if n} == {SHARED: 1}, name
    for f in ("pow_pool.hip", SRC):
        assert f'#include "{SHARED}"' in open(os.path.join(CSRC, f)).read()


def test_no_probe_spins():
    """Every probe loop is a for loop bounded by the table's size; the slot
    word is touched by atomics only in the insert, and nothing fences."""
    text = code()
    assert "while" not in text and "__threadfence" not in text and "volatile" not in text
    assert text.count(PROBE) == 3 and text.count("probe") == 3 * 3  # insert, join and scan, find
    for loop in re.findall(r"\bfor \([^)]*\)", text):
        assert loop == PROBE or re.fullmatch(r"for \(int (q = 0; q < 4; \+\+q|off = 32; off >= 1; off >>= 1)\)", loop), loop
    insert = text[text.index("void pow_pool_live_insert_kernel"):text.index("void pow_pool_live_join_kernel")]
    assert re.findall(r"\batomic\w+", insert) == ["atomicCAS", "atomicMin", "atomicOr"]
    assert "table[" not in insert.replace("&table[slot]", "")  # no plain access to a slot
    # nobody else writes the table
    rest = text[text.index("void pow_pool_live_join_kernel"):]
    assert not re.search(r"table\[[^\]]*\]\s*=[^=]", rest) and "atomicCAS" not in rest and "atomicMin" not in rest


def test_switches_only_in_the_test_library():
    shipped = open(_lib.LIB_PATH, "rb").read()
    test = open(_lib.TEST_LIB_PATH, "rb").read()
    for s in (b"POW_POOL_SLOTS_LOG2", b"POW_POOL_FIRST_CAP"):
        assert s not in shipped and s in test, s
    for f in os.listdir(CSRC):
        p = os.path.join(CSRC, f)
        if os.path.isfile(p) and f != "pow_hooks.cpp":
            assert 'getenv("POW_POOL' not in open(p).read(), f
    assert open(os.path.join(CSRC, "pow_hooks.cpp")).read().count('getenv("POW_POOL') == 2


def test_warmup_does_not_launch_the_kernels():
    assert "pow_launch_pool" not in api_function("pow_warmup")


def test_add_has_at_most_two_bounded_waits_and_no_work_per_earlier_block():
    """One tile walk over the new structs, then the fast path's timed section
    and, behind `if (adopted)`, the re-rank's.  Nothing on the host runs over
    the pool's earlier blocks and nothing goes up whose size depends on them."""
    body, h = pool_function("pow_pool_add"), timed_section_helpers()
    rank = pool_function("pow_queue_pool_rank", "hipError_t")
    assert h["timed_end"].count("stream_wait_for(") == 1
    assert body.count("verify_tiles(") == 1 and "pow_launch_pool_audit(ctx->stream" in body
    assert "ctx, blocks, m," in body[body.index("verify_tiles("):]  # the batch, not the pool
    after = body[body.index("[](const VerifyTile&) {}))"):]
    assert body.count("timed_begin(") == 2 and after.count("timed_begin(") == 2
    assert body.count("timed_end(") == 2 and after.count("timed_end(") == 2
    assert "stream_wait" not in body and "hipStreamSynchronize" not in body and "hipGraph" not in body
    fast, slow = after[:after.index("if (adopted) {")], after[after.index("if (adopted) {"):]
    assert fast.count("timed_begin(") == 1 and slow.count("timed_begin(") == 1
    order = [fast.index(s) for s in ("timed_begin(", "pow_launch_pool_live_insert(", "pow_launch_pool_live_join(",
                                     "pow_launch_pool_live_round(", "pow_launch_pool_live_finish(",
                                     "hipEventRecord(ctx->ev1", "hipMemcpyAsync(", "timed_end(")]
    assert order == sorted(order)
    order = [slow.index(s) for s in ("timed_begin(", "pow_launch_pool_live_strip(", "hipMemsetAsync(d_ctl, 0",
                                     "pow_launch_pool_join(", "pow_queue_pool_rank(ctx->stream, D, all)",
                                     "hipEventRecord(ctx->ev1", "hipMemcpyAsync(", "timed_end(")]
    assert order == sorted(order)
    # ... whose rank is K10's, stated once: the rounds, then the finish on the buffers the last round wrote
    order = [rank.index(s) for s in ("for (uint32_t r = 0; r < rounds; ++r)", "pow_launch_pool_round(stream, D, r)",
                                     "pow_launch_pool_finish(stream, D, rounds & 1u)")]
    assert order == sorted(order)
    assert "all = pow_pool_rounds(n)" in slow and "p->fin = all & 1u;" in slow
    # the only loops are the rounds': K11d's here, K10d's in the rank; no per-block host work
    assert re.findall(r"\bfor \(([^;]*);", body) == ["uint32_t r = 0"] and "while" not in body + rank
    assert re.findall(r"\bfor \(([^;]*);", rank) == ["uint32_t r = 0"]
    assert "padded_message" not in body and "std::vector" not in body
    # nothing goes up but the batch (verify_tiles) and resets; what comes down is the control words
    copies = re.findall(r"hipMemcpyAsync\(([^;]*);", body)
    assert len(copies) == 2 and all("sizeof(PowPoolLiveCtl), hipMemcpyDeviceToHost" in c for c in copies)
    grow = pool_function("pool_grow")
    assert grow.count("hipMemcpyAsync(") == 1 and "hipMemcpyDeviceToDevice" in grow and "HostToDevice" not in grow
    # the arrays and the table an add outgrows wait in d_old_* until the waits have passed
    assert grow.index("pool_retire(p->d_arr, p->d_old_arr, to.words)") < grow.index("hipMemcpyAsync(")
    order = [body.index(s) for s in ("pool_grow(p, n)", "pool_retire(p->d_table, p->d_old_table, slots)", "verify_tiles(",
                                     "if (adopted) {", "p->d_old_arr.release(), p->d_old_table.release();",
                                     "p->dead = false;")]
    assert order == sorted(order) and body.count("timed_end(") == 2
    assert body.rindex("timed_end(") < body.index("p->d_old_arr.release(), p->d_old_table.release();")
    # the argument checks come first, in the stated order
    checks = [body.index(s) for s in ("!p)", "!blocks && m", "m > POW_POOL_MAX_BLOCKS - p->size", "pool_ready(",
                                      "ctx->stats")]
    assert checks == sorted(checks)


def test_pool_buffers_are_released():
    """Every holder of pow_pool is named in its release_buffers, which open's failure path and close call."""
    api = open(os.path.join(CSRC, POOL_API)).read()
    struct = api[api.index("struct pow_pool {"):]
    struct = struct[:struct.index("\n};")]
    release = struct[struct.index("void release_buffers()"):]
    names = [n.strip() for decl in re.findall(r"^\s+(?:DevBuf|HostBuf)<[^>]+>\s+([^;]+);", struct, flags=re.M)
             for n in decl.split(",")]
    assert len(names) == 6
    for n in names:
        assert f"{n}.release()" in release, n
    assert api.count("p->release_buffers()") == 2
    assert "if (!ctx->wedged) p->release_buffers();" in pool_function("pow_pool_open")
    # the retired-buffer idiom has one statement and four users; the old holder is released by its caller alone
    retire = pool_function("pool_retire")
    order = [retire.index(s) for s in ("old = d_new;", "d_new = DevBuf<uint32_t>{};", "RESERVE(d_new, n);")]
    assert order == sorted(order) and "release" not in retire
    assert api.count("DevBuf<uint32_t>{}") == 1 and len(re.findall(r"\bpool_retire\(p->", api)) == 4
    assert api.count("p->d_old_arr.release(), p->d_old_table.release();") == 2
    assert "if (!ctx->wedged) p->release_buffers();" in api[api.index("void pow_pool_close("):]


def test_k10_is_as_it_was():
    """pow_pool.hip keeps its five kernels and launchers."""
    text = open(os.path.join(CSRC, "pow_pool.hip")).read()
    assert text.count("hipLaunchKernelGGL(") == 5 and text.count("__global__") == 5
