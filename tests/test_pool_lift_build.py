"""Codegen and source guards for K13, the kernels of pow_pool_ancestors,
pow_pool_fork_points and pow_pool_chain (csrc/pow_pool_lift.hip and
csrc/pow_lift_dev.h; CPU only: hipcc cross-compiles gfx950).  Metadata and
source checks only."""
import os
import re
import subprocess
import tempfile

import pytest

from mpi_blockchain_amd import _lib

from test_build import CSRC, POOL_API, ROOT, api_function, null_stream_calls, pool_function
from test_pool_build import kernel_metadata

SRC = "pow_pool_lift.hip"
SHARED = "pow_lift_dev.h"
KERNELS = {"row": "_Z24pow_pool_lift_row_kernel", "small": "_Z26pow_pool_lift_small_kernel",
           "ancestor": "_Z29pow_pool_lift_ancestor_kernel", "fork": "_Z25pow_pool_lift_fork_kernel"}
WITH_LDS = {"small": 2 * 256 * 4}  # K13b's hand-off: two halves of one word per lane
CALLS = {"pow_pool_ancestors": "pool_lift_args(", "pow_pool_fork_points": "pool_lift_args(", "pow_pool_chain": None}
BOUND = r"uint32_t [jk] = [01]; [jk] < POW_LIFT_MAX_LEVELS; \+\+[jk]"  # every loop of both files


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


def code(f: str = SRC) -> str:
    return re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, f)).read())


@pytest.mark.parametrize("which", sorted(KERNELS))
def test_lift_kernels_have_no_scratch_and_no_spills(isa, which):
    md = kernel_metadata(isa, KERNELS[which])
    assert md["private_segment_fixed_size"] == 0, md
    assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md
    assert md["wavefront_size"] == 64 and md["vgpr_count"] <= 64, md
    assert md["group_segment_fixed_size"] == WITH_LDS.get(which, 0), md  # LDS in K13b only


def test_lift_kernels_are_in_both_libraries():
    from mpi_blockchain_amd import build

    for test in (False, True):
        assert os.path.join(CSRC, SRC) in build.sources(test=test)
    assert SRC not in build.TEST_ONLY and SHARED in build.HEADERS
    for path in (_lib.LIB_PATH, _lib.TEST_LIB_PATH):
        lib = open(path, "rb").read()
        for k in KERNELS.values():
            assert k.encode() in lib, (path, k)


def test_no_null_stream_in_lift_sources():
    kernel = open(os.path.join(CSRC, SRC)).read()
    assert not null_stream_calls(kernel)
    assert kernel.count("hipLaunchKernelGGL(") == 4 and kernel.count("__global__") == 4
    assert "<<<" not in kernel and "hipGraph" not in kernel
    assert kernel.count("__launch_bounds__(256)") == 4 and kernel.count("dim3(256), 0, stream") == 4
    bodies = {name: pool_function(name) for name in ("pow_pool_ancestors", "pow_pool_fork_points", "pow_pool_chain",
                                                     "pow_pool_lift_get_info", "pool_lift_args", "pool_lift_update",
                                                     "pool_lift_run", "pool_lift_ready")}
    bodies["pow_queue_pool_lift"] = pool_function("pow_queue_pool_lift", "hipError_t")
    for name, body in bodies.items():
        assert not null_stream_calls(body), name
        assert "hipStreamSynchronize" not in body and "hipDeviceSynchronize" not in body and "hipGraph" not in body, name


def test_no_spins_no_fences_no_atomics_and_constant_bounds():
    for f in (SRC, SHARED):
        text = code(f)
        assert "while" not in text and "__threadfence" not in text and "volatile" not in text, f
        assert "atomic" not in text and "__shfl" not in text, f
        assert "rocprim" not in text and "hipcub" not in text and "thrust" not in text, f
        loops = re.findall(r"\bfor \(([^)]*)\)", text)
        assert loops, f
        for loop in loops:
            assert re.fullmatch(BOUND, loop), (f, loop)
    assert code(SRC).count("__syncthreads()") == 1  # K13b's one barrier per level
    assert f'#include "{SHARED}"' in open(os.path.join(CSRC, SRC)).read()


def test_the_walks_have_one_copy_and_compile_on_the_host():
    """ancestor, fork point and a row's entry are written once, in the shared
    header, behind a macro that a host compiler sees as plain inline."""
    shared = open(os.path.join(CSRC, SHARED)).read()
    for name in ("pow_lift_entry", "pow_lift_jump", "pow_lift_ancestor", "pow_lift_fork"):
        definition = re.compile(rf"^POW_LIFT_FN[^\n;=#/]*\b{name}\s*\(", flags=re.M)
        assert len(definition.findall(shared)) == 1, name
        assert f"{name}(" in code(SRC) or name == "pow_lift_jump"
    assert "#define POW_LIFT_FN __host__ __device__ inline" in shared and "#define POW_LIFT_FN inline" in shared
    assert "hip/" not in shared
    # every position taken from the table is compared with size before it indexes anything
    kernels = code(SRC)
    assert "if (x < v.size && y < v.size)" in kernels and "at < v.size ?" in kernels and "tip < v.size ?" in kernels
    assert "if (mine < size)" in kernels and "& 255u" in kernels


def test_warmup_does_not_launch_the_kernels():
    assert "pow_launch_pool" not in api_function("pow_warmup")


def test_the_host_side_of_the_query_calls():
    """Each call: its argument checks, pool_ready, then one pool_lift_run, which
    holds the one timed section.  No host loop but the position check (over the
    queries) and the table's rows."""
    args, update, run = pool_function("pool_lift_args"), pool_function("pool_lift_update"), pool_function("pool_lift_run")
    queue = pool_function("pow_queue_pool_lift", "hipError_t")  # the table's launches, stated once
    assert re.findall(r"\bfor \(([^;]*);", args) == ["size_t q = 0"] and "q < k" in args
    assert re.findall(r"\bfor \(([^;]*);", queue) == ["uint32_t j = 1", "uint32_t j = have + 1u"]  # rows, never blocks
    assert "for (" not in run + update and "while" not in run + update + args + queue
    assert run.count("timed_begin(") == 1 and run.count("timed_end(") == 1 and "timed_" not in update + queue
    assert update.count("pow_queue_pool_lift(") == 1 and "pow_launch_pool" not in update
    assert "stream_wait" not in queue and "hipEvent" not in queue and "hipMemcpy" not in queue and "ctx" not in queue
    # K13b for at most POW_POOL_LIFT_SMALL new blocks, else K13a per old row over them; then every new row over all
    order = [queue.index(s) for s in ("if (m && have) {", "if (m <= POW_POOL_LIFT_SMALL) {",
                                      "pow_launch_pool_lift_small(stream, parent, up, capacity, have, covered, n)",
                                      "for (uint32_t j = 1; j <= have;",
                                      "pow_launch_pool_lift_row(stream, parent, up, capacity, j, covered, m, n)",
                                      "for (uint32_t j = have + 1u; j <= rows;",
                                      "pow_launch_pool_lift_row(stream, parent, up, capacity, j, 0, n, n)")]
    assert order == sorted(order)
    assert "have = stale ? 0u : pow_pool_lift_rows(covered), rows = pow_pool_lift_rows(n)" in queue
    assert run.count("hipMemcpyAsync(") == 2  # the arguments up in one copy, the results down in one
    order = [run.index(s) for s in ("pool_lift_ready(p, &covered, &stale)", "RESERVE(p->d_find", "hipMemcpyHostToDevice",
                                    "timed_begin(", "pool_lift_update(", "pow_launch_pool_lift_fork(",
                                    "pow_launch_pool_lift_ancestor(", "hipEventRecord(ctx->ev1", "hipMemcpyDeviceToHost",
                                    "timed_end(", "pool_lift_commit(p);")]
    assert order == sorted(order)
    # the table's step, stated once for this run and K14's: made ready in front of the timed section (what the update
    # starts from, the table at the pool's capacity, nothing covered meanwhile), committed behind the wait
    ready, commit = pool_function("pool_lift_ready"), api_function("pool_lift_commit", POOL_API, "void")
    stale = api_function("pool_lift_stale", POOL_API, "bool")
    order = [ready.index(s) for s in ("*stale = pool_lift_stale(p);", "if (t.capacity < p->plan.cap) {", "t.release_table();",
                                      "RESERVE(t.d_up, (size_t)p->plan.cap * pow_pool_lift_rows(p->plan.cap));",
                                      "t.capacity = p->plan.cap;", "*covered = *stale ? 0u : t.covered;", "t.covered = 0;")]
    assert order == sorted(order) and "timed_" not in ready + commit + stale and "for (" not in ready + commit + stale
    assert "p->lift.covered = p->size;" in commit and "p->lift.gen = p->gen;" in commit
    assert "t.covered == 0 || t.capacity == 0 || t.gen != p->gen || t.covered > p->size || p->plan.cap > t.capacity" in stale
    api = open(os.path.join(CSRC, POOL_API)).read()
    assert api.count("t.gen != p->gen") == 1 and len(re.findall(r"\bgen [!=]= p->gen", api)) == 1  # one predicate
    assert api.count("pool_lift_stale(p)") == 2 and api.count("RESERVE(t.d_up") == 1
    for user in (run, pool_function("pool_above_run")):
        assert user.count("pool_lift_ready(") == 1 and user.count("pool_lift_commit(") == 1
        assert user.index("pool_lift_ready(") < user.index("RESERVE(p->d_find") < user.index("timed_begin(")
        assert user.index("timed_end(") < user.index("pool_lift_commit(")
        assert "t.gen" not in user and "t.covered" not in user and "release_table" not in user
    # pow_stats.launches is the count of what was queued: every launcher call in the sequence is counted exactly
    # once, and pool_lift_run hands that count (and the query launch) to timed_end ...
    launchers = re.findall(r"pow_launch_pool_lift_\w+\(", queue)
    assert len(launchers) == 3 and len(re.findall(r"\+\+\*launches", queue)) == len(launchers)
    assert len(re.findall(r"\*?\blaunches\b", queue)) == 1 + len(launchers)  # the parameter, then one increment each
    assert re.search(r"pow_launch_pool_lift_small\([^;]*;\s+\+\+\*launches;", queue)  # K13b: once
    assert len(re.findall(r"\+\+j, \+\+\*launches\)\s+QUEUE_OK\(pow_launch_pool_lift_row\(", queue)) == 2  # K13a: once a row
    assert "uint32_t launches = 0;" in run and "pool_lift_update(p, covered, stale, &launches, &work)" in run
    assert "launches + 1u, &ctx->stats" in run and len(re.findall(r"\blaunches\b", re.sub(r"//[^\n]*", "", run))) == 3
    assert "launches" not in update.replace("uint32_t* launches", "").replace("stale, launches,", "")
    # ... and the closed form the plan unit and Python restate has its one definition, in pow_host.cpp
    defs = {f: len(re.findall(r"^uint32_t pow_pool_lift_launches\([^;{]*\) \{", open(os.path.join(CSRC, f)).read(), flags=re.M))
            for f in os.listdir(CSRC) if os.path.isfile(os.path.join(CSRC, f))}
    assert {f: n for f, n in defs.items() if n} == {"pow_host.cpp": 1}
    assert "pow_pool_lift_launches" not in open(os.path.join(CSRC, POOL_API)).read()  # the calls count, they do not restate
    for name, checks in CALLS.items():
        body = pool_function(name)
        assert "for (" not in body and "while" not in body and "std::vector" not in body, name
        assert body.count("pool_lift_run(") == 1 and "timed_begin(" not in body and "hipMalloc" not in body, name
        first = "!p)" if checks is None else checks
        order = [body.index(s) for s in (first, "pool_ready(", "ctx->stats = pow_stats{}", "if (k == 0) return POW_OK;",
                                         "pool_lift_run(")]
        assert order == sorted(order), name
    info = pool_function("pow_pool_lift_get_info")
    assert "hip" not in info and "ctx" not in info  # no GPU work
    assert "covered = pool_lift_stale(p) ? 0u : t.covered;" in info and "gen" not in info  # fresh by the same predicate


def test_the_table_is_one_member_and_the_generation_has_two_bumps():
    api = open(os.path.join(CSRC, POOL_API)).read()
    struct = api[api.index("struct pow_pool {"):]
    struct = struct[:struct.index("\n};")]
    assert struct.count("PowPoolLift lift;") == 1 and "lift.release();" in struct[struct.index("void release_buffers()"):]
    assert api.count("++p->gen") == 2
    fill = api[api.index("static void pool_fill_info("):]
    assert "if (reranked) ++p->gen;" in fill[:fill.index("\n}\n")]
    compact = pool_function("pool_compact")  # the prune's second half, and the drop's
    assert compact.count("p->lift.release_table(), ++p->gen;") == 1  # it gives the table's memory back
    assert api.count("p->lift.release_table(), ++p->gen;") == 1
    assert compact.index("timed_end(") < compact.index("p->lift.release_table(), ++p->gen;") < compact.index("p->size = kept;")
    add = pool_function("pow_pool_add")
    assert "lift" not in add and "gen" not in add  # the add launches nothing new: the bump is pool_fill_info's
