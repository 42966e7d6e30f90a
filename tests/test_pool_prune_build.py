"""Codegen and source guards for K12, the kernels of pow_pool_mark and
pow_pool_prune (csrc/pow_pool_prune.hip; CPU only: hipcc cross-compiles
gfx950).  Metadata and source checks only."""
import os
import re
import subprocess
import tempfile

import pytest

from mpi_blockchain_amd import _lib

from test_build import CSRC, POOL_API, ROOT, api_function, null_stream_calls, pool_function

QUEUES = ("pow_queue_pool_mark", "pow_queue_pool_compact")  # the K12 sequences pow_api.cpp states once
from test_pool_build import kernel_metadata

SRC = "pow_pool_prune.hip"
KERNELS = {"seed": "_Z26pow_pool_prune_seed_kernel", "round": "_Z27pow_pool_prune_round_kernel",
           "count": "_Z27pow_pool_prune_count_kernel", "scan": "_Z26pow_pool_prune_scan_kernel",
           "gather": "_Z28pow_pool_prune_gather_kernel", "remap": "_Z27pow_pool_prune_remap_kernel"}
WITH_LDS = {"scan": 16, "gather": 16}  # four wave totals each


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
def test_prune_kernels_have_no_scratch_and_no_spills(isa, which):
    md = kernel_metadata(isa, KERNELS[which])
    assert md["private_segment_fixed_size"] == 0, md
    assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md
    assert md["wavefront_size"] == 64 and md["vgpr_count"] <= 64, md
    assert md["group_segment_fixed_size"] == WITH_LDS.get(which, 0), md  # LDS in the scan and the gather only
    m = re.search(rf"^({KERNELS[which]}\w*):[^\n]*\n(.*?)s_endpgm", isa, flags=re.S | re.M)
    assert m and not re.search(r"^\s+scratch_", m.group(2), flags=re.M)


def test_prune_kernels_are_in_both_libraries():
    from mpi_blockchain_amd import build

    for test in (False, True):
        assert os.path.join(CSRC, SRC) in build.sources(test=test)
    assert SRC not in build.TEST_ONLY
    for path in (_lib.LIB_PATH, _lib.TEST_LIB_PATH):
        lib = open(path, "rb").read()
        for k in KERNELS.values():
            assert k.encode() in lib, (path, k)


def test_no_null_stream_in_prune_sources():
    kernel = open(os.path.join(CSRC, SRC)).read()
    assert not null_stream_calls(kernel)
    assert kernel.count("hipLaunchKernelGGL(") == 6 and kernel.count("__global__") == 6
    assert "<<<" not in kernel and "hipGraph" not in kernel
    assert kernel.count("__launch_bounds__(256)") == 6 and kernel.count("dim3(256), 0, stream") == 6
    bodies = {name: pool_function(name) for name in ("pow_pool_mark", "pow_pool_prune", "pool_mark_run", "pool_mark_args",
                                                     "pool_compact")}
    bodies.update({name: pool_function(name, "hipError_t") for name in QUEUES})
    for name, body in bodies.items():
        assert not null_stream_calls(body), name
        assert "hipStreamSynchronize" not in body and "hipDeviceSynchronize" not in body and "hipGraph" not in body, name


def test_no_spins_no_fences_and_wave64_idioms():
    text = code()
    assert "while" not in text and "__threadfence" not in text and "volatile" not in text
    assert "rocprim" not in text and "hipcub" not in text and "thrust" not in text  # the scan is the file's own
    assert "__ballot(" in text and "__shfl_xor(" in text and "__shfl_up(" in text
    # every loop has constant bounds
    for loop in re.findall(r"\bfor \([^)]*\)", text):
        assert re.fullmatch(r"for \((int off = 32; off >= 1; off >>= 1|int off = 1; off <= 32; off <<= 1|"
                            r"int k = 0; k < 16; \+\+k|uint32_t w = 0; w < [34]; \+\+w)\)", loop), loop
    # the only atomics are K10e's two, in the remap
    remap = text[text.index("void pow_pool_prune_remap_kernel"):text.index("hipError_t pow_launch_pool_prune_seed")]
    assert re.findall(r"\batomic\w+", text) == re.findall(r"\batomic\w+", remap) == ["atomicMax", "atomicAdd"]
    # a mark is only ever set: every store to it writes 1
    assert re.findall(r"mark\[[^\]]*\]\s*=[^=][^;]*;", text) == ["mark[i] = 1;", "mark[t] = 1;", "mark[nx] = 1;"]


def test_the_rounds_go_ping_pong():
    """The coverage argument needs equal jump lengths: a round reads one next
    buffer and writes the other, never in place."""
    text = code()
    kernel = text[text.index("void pow_pool_prune_round_kernel"):text.index("void pow_pool_prune_count_kernel")]
    assert "next_b[i] = nx;" in kernel and not re.search(r"next_a\[[^\]]*\]\s*=[^=]", kernel)
    launcher = text[text.index("hipError_t pow_launch_pool_prune_round"):text.index("hipError_t pow_launch_pool_prune_count")]
    assert "D.next[a]" in launcher and "D.next[a ^ 1u]" in launcher
    mark = pool_function("pow_queue_pool_mark", "hipError_t")
    assert "for (uint32_t r = 0; r < rounds; ++r) QUEUE_OK(pow_launch_pool_prune_round(stream, D, fin, r));" in mark
    assert "rounds = pow_pool_rounds(D.n)" in mark
    run = pool_function("pool_mark_run")  # its D holds the pool's blocks, and its budget counts the same rounds
    assert "n = p->size, rounds = pow_pool_rounds(n)" in run and "D = pool_dev(p, n)" in run


def test_warmup_does_not_launch_the_kernels():
    assert "pow_launch_pool" not in api_function("pow_warmup")


def test_the_pool_has_no_new_holder_and_k10_k11_are_as_they_were():
    api = open(os.path.join(CSRC, POOL_API)).read()
    struct = api[api.index("struct pow_pool {"):]
    struct = struct[:struct.index("\n};")]
    names = [n.strip() for decl in re.findall(r"^\s+(?:DevBuf|HostBuf)<[^>]+>\s+([^;]+);", struct, flags=re.M)
             for n in decl.split(",")]
    assert names == ["d_arr", "d_table", "d_old_arr", "d_old_table", "d_find", "h_ctl"]
    assert api.count("p->release_buffers()") == 2
    for f, launches in (("pow_pool.hip", 5), ("pow_pool_live.hip", 6)):
        text = open(os.path.join(CSRC, f)).read()
        assert text.count("hipLaunchKernelGGL(") == launches and text.count("__global__") == launches, f


def test_the_host_side_of_both_calls():
    """mark: one timed section.  prune: that one and, if it drops and keeps,
    a second (pool_compact); the old arrays wait until its wait has passed.  No host loop
    runs over the pool's blocks: the one loop is the check of the tips."""
    args, run = pool_function("pool_mark_args"), pool_function("pool_mark_run")
    mark, prune, compact = pool_function("pow_pool_mark"), pool_function("pow_pool_prune"), pool_function("pool_compact")
    q_mark, q_compact = (pool_function(name, "hipError_t") for name in QUEUES)
    assert re.findall(r"\bfor \(([^;]*);", args) == ["size_t k = 0"] and "k < n_tips" in args
    assert re.findall(r"\bfor \(([^;]*);", q_mark) == ["uint32_t r = 0"]
    for body in (mark, prune, compact, run, q_compact):
        assert "for (" not in body and "while" not in body and "std::vector" not in body and "std::iota" not in body
    assert run.count("timed_begin(") == 1 and run.count("timed_end(") == 1
    # the caller's part of the mark's section ...
    order = [run.index(s) for s in ("hipMemcpyHostToDevice", "timed_begin(",
                                    "pow_queue_pool_mark(ctx->stream, D, p->fin, p->d_find.p, n_tips, min_index, flags)",
                                    "hipEventRecord(ctx->ev1", "hipMemcpyDeviceToHost", "timed_end(")]
    assert order == sorted(order)
    # ... and the sequence's: the reset and the launches in their order; it waits for nothing and times nothing
    order = [q_mark.index(s) for s in ("rounds = pow_pool_rounds(", "hipMemsetAsync(D.depth[fin ^ 1u], 0",
                                       "pow_launch_pool_prune_seed(", "for (uint32_t r = 0; r < rounds; ++r)",
                                       "pow_launch_pool_prune_round(", "pow_launch_pool_prune_count(",
                                       "pow_launch_pool_prune_scan(")]
    assert order == sorted(order)
    for body in (q_mark, q_compact):
        assert "timed_" not in body and "stream_wait" not in body and "hipEvent" not in body and "hipMemcpy" not in body
        assert "ctx" not in body and "pow_pool*" not in body  # a stream and views, never a pool
    assert "3u + rounds, &ctx->stats" in run
    assert mark.count("pool_mark_run(") == 1 and "timed_begin(" not in mark and "hipMalloc" not in mark
    assert prune.count("pool_mark_run(") == 1 and "timed_" not in prune and "pool_retire(" not in prune
    assert compact.count("timed_begin(") == 1 and compact.count("timed_end(") == 1 and "p->dead" not in compact
    order = [prune.index(s) for s in ("pool_mark_run(", "if (kept >= n) {", "} else if (int rc = pool_compact(p, kept, map)) {",
                                      "p->dead = false;", "return pool_result(p, info);")]
    assert order == sorted(order) and prune.count("pool_compact(") == 1
    order = [compact.index(s) for s in ("pool_retire(p->d_arr, p->d_old_arr, to.words)",
                                        "pool_retire(p->d_table, p->d_old_table, slots)", "timed_begin(",
                                        "pow_queue_pool_compact(ctx->stream, F, T, cap, p->fin, map != nullptr)",
                                        "hipEventRecord(ctx->ev1",
                                        "sizeof(PowPoolLiveCtl), hipMemcpyDeviceToHost", "timed_end(",
                                        "p->d_old_arr.release(), p->d_old_table.release();", "p->size = kept;",
                                        "pool_fill_info(p, *ctl, 0, false, true);")]
    assert order == sorted(order)
    retire = pool_function("pool_retire")  # what each of the two lines above does: the old buffer kept, a new one made
    order = [retire.index(s) for s in ("old = d_new;", "d_new = DevBuf<uint32_t>{};", "RESERVE(d_new, n);")]
    assert order == sorted(order)
    order = [q_compact.index(s) for s in ("hipMemsetAsync(T.ctl, 0", "if (T.table) QUEUE_OK(hipMemsetAsync(T.table, 0xFF",
                                          "if (T.n) {", "pow_launch_pool_prune_gather(", "pow_launch_pool_prune_remap(",
                                          "if (T.table) QUEUE_OK(pow_launch_pool_insert(stream, T))",
                                          "} else if (want_map) {", "hipMemsetD32Async((hipDeviceptr_t)F.next[0], (int)POW_POOL_NONE, F.n")]
    assert order == sorted(order)
    # the compaction's T is the survivors' view with the new table: T.n = kept, T.slots = slots
    assert "T = pow_pool_live_dev(p->d_arr.p, to, p->d_table.p, kept, slots)" in compact
    assert "pow_pool_prune_cap(kept, pow_pool_live_first_cap(0, ctx->pool_first_cap))" in compact
    assert "pow_pool_prune_slots(cap, kept, ctx->pool_slots_log2)" in compact
    for body in (prune, compact):  # no struct goes up
        assert "HostToDevice" not in body and "padded_message" not in body and "verify_tiles" not in body
    assert prune.index("p->dead = true;") < prune.index("pool_mark_run(")
