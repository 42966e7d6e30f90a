"""Codegen and source guards for K12, the kernels of pow_pool_mark and
pow_pool_prune (csrc/pow_pool_prune.hip; CPU only: hipcc cross-compiles
gfx950).  Metadata and source checks only."""
import os
import re
import subprocess
import tempfile

import pytest

from mpi_blockchain_amd import _lib

from test_build import CSRC, ROOT, api_function, null_stream_calls
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
    for name in ("pow_pool_mark", "pow_pool_prune", "pool_mark_run", "pool_mark_args"):
        body = api_function(name)
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
    run = api_function("pool_mark_run")
    assert "for (uint32_t r = 0; r < rounds; ++r) HIP_OK(pow_launch_pool_prune_round(ctx->stream, D, p->fin, r));" in run
    assert "rounds = pow_pool_rounds(n)" in run


def test_warmup_does_not_launch_the_kernels():
    assert "pow_launch_pool" not in api_function("pow_warmup")


def test_the_pool_has_no_new_holder_and_k10_k11_are_as_they_were():
    api = open(os.path.join(CSRC, "pow_api.cpp")).read()
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
    a second; the old arrays wait until its wait has passed.  No host loop
    runs over the pool's blocks: the one loop is the check of the tips."""
    args, run = api_function("pool_mark_args"), api_function("pool_mark_run")
    mark, prune = api_function("pow_pool_mark"), api_function("pow_pool_prune")
    assert re.findall(r"\bfor \(([^;]*);", args) == ["size_t k = 0"] and "k < n_tips" in args
    assert re.findall(r"\bfor \(([^;]*);", run) == ["uint32_t r = 0"]
    for body in (mark, prune):
        assert "for (" not in body and "while" not in body and "std::vector" not in body and "std::iota" not in body
    assert run.count("timed_begin(") == 1 and run.count("timed_end(") == 1
    order = [run.index(s) for s in ("hipMemcpyHostToDevice", "timed_begin(", "hipMemsetAsync(", "pow_launch_pool_prune_seed(",
                                    "pow_launch_pool_prune_round(", "pow_launch_pool_prune_count(",
                                    "pow_launch_pool_prune_scan(", "hipEventRecord(ctx->ev1", "hipMemcpyDeviceToHost",
                                    "timed_end(")]
    assert order == sorted(order)
    assert "3u + rounds, &ctx->stats" in run
    assert mark.count("pool_mark_run(") == 1 and "timed_begin(" not in mark and "hipMalloc" not in mark
    assert prune.count("pool_mark_run(") == 1 and prune.count("timed_begin(") == 1 and prune.count("timed_end(") == 1
    order = [prune.index(s) for s in ("pool_mark_run(", "p->d_old_arr = p->d_arr;", "RESERVE(p->d_arr", "p->d_old_table = p->d_table;",
                                      "RESERVE(p->d_table", "timed_begin(", "hipMemsetAsync(T.ctl, 0", "hipMemsetAsync(T.table, 0xFF",
                                      "pow_launch_pool_prune_gather(", "pow_launch_pool_prune_remap(",
                                      "pow_launch_pool_insert(ctx->stream, T)", "hipEventRecord(ctx->ev1",
                                      "sizeof(PowPoolLiveCtl), hipMemcpyDeviceToHost", "timed_end(",
                                      "p->d_old_arr.release(), p->d_old_table.release();", "p->dead = false;")]
    assert order == sorted(order)
    assert "pow_pool_prune_cap(kept, pow_pool_live_first_cap(0, ctx->pool_first_cap))" in prune
    assert "pow_pool_prune_slots(cap, kept, ctx->pool_slots_log2)" in prune
    assert "HostToDevice" not in prune and "padded_message" not in prune and "verify_tiles" not in prune  # no struct goes up
    assert prune.index("p->dead = true;") < prune.index("pool_mark_run(")
