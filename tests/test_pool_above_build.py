"""Codegen and source guards for K14, the kernels of pow_pool_tips,
pow_pool_subtrees and pow_pool_drop (csrc/pow_pool_above.hip and
csrc/pow_above_dev.h; CPU only: hipcc cross-compiles gfx950).  Metadata and
source checks only."""
import os
import re
import subprocess
import tempfile

import pytest

from mpi_blockchain_amd import _lib

from test_build import CSRC, ROOT, api_function, null_stream_calls, pool_function
from test_pool_build import kernel_metadata

SRC = "pow_pool_above.hip"
SHARED = "pow_above_dev.h"
KERNELS = {"child": "_Z27pow_pool_above_child_kernel", "tip": "_Z25pow_pool_above_tip_kernel",
           "gather": "_Z28pow_pool_above_gather_kernel", "subtree": "_Z29pow_pool_above_subtree_kernel"}
WITH_LDS = {"gather": 4 * 4}  # K14c's four wave counts
LOOPS = (r"int off = 32; off >= 1; off >>= 1", r"uint32_t w = 0; w < 3; \+\+w")
QUEUES = ("pow_queue_pool_tips", "pow_queue_pool_above")


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
def test_above_kernels_have_no_scratch_and_no_spills(isa, which):
    md = kernel_metadata(isa, KERNELS[which])
    assert md["private_segment_fixed_size"] == 0, md
    assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md
    assert md["wavefront_size"] == 64 and md["vgpr_count"] <= 64, md
    assert md["group_segment_fixed_size"] == WITH_LDS.get(which, 0), md  # LDS in K14c only
    m = re.search(rf"^({KERNELS[which]}\w*):[^\n]*\n(.*?)s_endpgm", isa, flags=re.S | re.M)
    assert m and not re.search(r"^\s+scratch_", m.group(2), flags=re.M)


def test_above_kernels_are_in_both_libraries():
    from mpi_blockchain_amd import build

    for test in (False, True):
        assert os.path.join(CSRC, SRC) in build.sources(test=test)
    assert SRC not in build.TEST_ONLY and SHARED in build.HEADERS
    for path in (_lib.LIB_PATH, _lib.TEST_LIB_PATH):
        lib = open(path, "rb").read()
        for k in KERNELS.values():
            assert k.encode() in lib, (path, k)


def test_no_null_stream_in_above_sources():
    kernel = open(os.path.join(CSRC, SRC)).read()
    assert not null_stream_calls(kernel)
    assert kernel.count("hipLaunchKernelGGL(") == 4 and kernel.count("__global__") == 4
    assert "<<<" not in kernel and "hipGraph" not in kernel
    assert kernel.count("__launch_bounds__(256)") == 4 and kernel.count("dim3(256), 0, stream") == 4
    bodies = {name: pool_function(name) for name in ("pow_pool_tips", "pow_pool_subtrees", "pow_pool_drop",
                                                     "pool_above_args", "pool_above_run")}
    bodies.update({name: pool_function(name, "hipError_t") for name in QUEUES})
    for name, body in bodies.items():
        assert not null_stream_calls(body), name
        assert "hipStreamSynchronize" not in body and "hipDeviceSynchronize" not in body and "hipGraph" not in body, name


def test_no_spins_no_fences_and_constant_bounds():
    for f in (SRC, SHARED):
        text = code(f)
        assert "while" not in text and "__threadfence" not in text and "volatile" not in text, f
        assert "rocprim" not in text and "hipcub" not in text and "thrust" not in text, f
        for loop in re.findall(r"\bfor \(([^)]*)\)", text):
            assert any(re.fullmatch(b, loop) for b in LOOPS), (f, loop)
    text = code()
    assert len(re.findall(r"\bfor \(", text)) == 2 and "for (" not in code(SHARED)  # the jump's loop is pow_lift_jump's
    assert text.count("__syncthreads()") == 1  # K14c's, between the wave counts and the ranks
    # the only atomics are the subtree kernel's three, into its root's record
    subtree = text[text.index("void pow_pool_above_subtree_kernel"):text.index("static_assert(POW_LIFT_NONE")]
    assert re.findall(r"\batomic\w+", text) == re.findall(r"\batomic\w+", subtree) == ["atomicAdd", "atomicMax", "atomicMax"]
    # every store to a mark: K14a sets, K14b rewrites its own, K14d stores the launch's value
    assert re.findall(r"(?:mark|has_child)\[[^\]]*\]\s*=[^=][^;]*;", text) == \
        ["has_child[par] = 1;", "mark[i] = tip ? 1 : 0;", "mark[i] = (uint8_t)value;"]
    # every position read is compared with the size before it indexes anything
    assert "if (par < n) has_child[par] = 1;" in text and "if (on && j < room) list[j] = i;" in text
    assert "if (r < v.size && pow_above_member(v, i, r))" in text and "q < k ? roots[q] : POW_POOL_NONE" in text
    head = open(os.path.join(CSRC, SRC)).read()
    assert "// Memory ordering." in head[:head.index("#include")] and f'#include "{SHARED}"' in head


def test_the_member_test_has_one_copy_and_compiles_on_the_host():
    shared = open(os.path.join(CSRC, SHARED)).read()
    assert len(re.findall(r"^POW_LIFT_FN[^\n;=#/]*\bpow_above_member\s*\(", shared, flags=re.M)) == 1
    assert '#include "pow_lift_dev.h"' in shared and "hip/" not in shared and "__global__" not in shared
    assert "return di >= dr && pow_lift_jump(v, i, di - dr) == r;" in code(SHARED)
    assert code().count("pow_above_member(") == 1 and "pow_lift_jump" not in code()


def test_the_untouched_files_and_the_reused_wrappers():
    """K12c, K12d, the compaction and the table's update are the ones there were."""
    text = code()
    count = text[text.index("hipError_t pow_launch_pool_above_count"):text.index("hipError_t pow_launch_pool_above_gather")]
    assert count.index("pow_launch_pool_prune_count(stream, D, fin)") < count.index("pow_launch_pool_prune_scan(stream, D)")
    run, drop = pool_function("pool_above_run"), pool_function("pow_pool_drop")
    assert run.count("pool_lift_update(p, covered, stale, &launches, &work)") == 1
    assert "pow_queue_pool_compact" not in drop and "pow_pool_prune(" not in drop
    assert drop.count("pool_compact(p, kept, map)") == 1  # the prune's own second half, called as the prune calls it
    assert "hip" not in drop[drop.index("if (k == 0) {"):drop.index("uint32_t kept = 0;")]  # no roots: no GPU work
    for f, launches in (("pow_pool_prune.hip", 6), ("pow_pool_lift.hip", 4)):
        t = open(os.path.join(CSRC, f)).read()
        assert t.count("hipLaunchKernelGGL(") == launches and t.count("__global__") == launches, f


def test_warmup_does_not_launch_the_kernels():
    assert "pow_launch_pool" not in api_function("pow_warmup") and "pow_queue_pool" not in api_function("pow_warmup")


def test_the_host_side_of_the_three_calls():
    """tips: one timed section.  subtrees: one, pool_above_run's.  drop: that
    one and pool_compact's.  No host loop runs over the pool's blocks: the loops
    are over the roots."""
    tips, subtrees, drop = (pool_function(n) for n in ("pow_pool_tips", "pow_pool_subtrees", "pow_pool_drop"))
    args, run = pool_function("pool_above_args"), pool_function("pool_above_run")
    q_tips, q_above = (pool_function(n, "hipError_t") for n in QUEUES)
    assert re.findall(r"\bfor \(([^;]*);", args) == ["size_t q = 0"] and "q < k" in args
    assert re.findall(r"\bfor \(([^;]*);", subtrees) == ["size_t q = 0"] and "q < k" in subtrees
    for body in (tips, drop, run, q_tips, q_above):
        assert "for (" not in body and "while" not in body and "std::vector" not in body
    for body in (tips, run):
        assert body.count("timed_begin(") == 1 and body.count("timed_end(") == 1
    for body in (subtrees, drop):
        assert "timed_" not in body and body.count("pool_above_run(") == 1 and "hipMalloc" not in body
    for body in (q_tips, q_above):
        assert "timed_" not in body and "stream_wait" not in body and "hipEvent" not in body and "hipMemcpy" not in body
        assert "ctx" not in body and "pow_pool*" not in body  # a stream and views, never a pool
    # the argument checks in the header's order, then the pool's readiness, before anything is written
    order = [tips.index(s) for s in ("!p)", "~(unsigned)POW_TIPS_SOUND_ONLY", "!n_tips || (!out && cap)", "pool_ready(",
                                     "ctx->stats = pow_stats{}", "*n_tips = 0;", "timed_begin(",
                                     "pow_queue_pool_tips(ctx->stream, D, p->fin, flags)", "hipEventRecord(ctx->ev1",
                                     "timed_end(", "memcpy(out,", "POW_ENOSPC")]
    assert order == sorted(order) and "5u, &ctx->stats" in tips
    order = [args.index(s) for s in ("k > POW_POOL_MAX_ROOTS", "!roots && k", "roots[q] >= p->size")]
    assert order == sorted(order)
    for body in (subtrees, drop):
        order = [body.index(s) for s in ("!p)", "pool_above_args(p, roots, k)", "pool_ready(", "ctx->stats = pow_stats{}",
                                         "pool_above_run(")]
        assert order == sorted(order)
    # the table's step is the K13 queries' (test_pool_lift_build holds its two halves): once in front, once behind
    order = [run.index(s) for s in ("pool_lift_ready(p, &covered, &stale)", "RESERVE(p->d_find", "hipMemcpyHostToDevice",
                                    "timed_begin(", "pool_lift_update(", "pow_queue_pool_above(", "hipEventRecord(ctx->ev1",
                                    "hipMemcpyDeviceToHost", "timed_end(", "pool_lift_commit(p);")]
    assert order == sorted(order) and "launches + (marks ? 3u : 1u), &ctx->stats" in run
    assert run.count("pool_lift_ready(") == 1 and run.count("pool_lift_commit(") == 1
    assert "RESERVE(t.d_up" in pool_function("pool_lift_ready") and "t.gen" not in run and "t.covered" not in run
    # the sequences: resets in front, K12c and K12d behind the marks
    order = [q_tips.index(s) for s in ("hipMemsetAsync(D.depth[fin ^ 1u], 0", "pow_launch_pool_above_child(",
                                       "pow_launch_pool_above_tip(", "pow_launch_pool_above_count(",
                                       "pow_launch_pool_above_gather(")]
    assert order == sorted(order)
    order = [q_above.index(s) for s in ("hipMemsetAsync(d_acc, 0", "hipMemsetAsync(D.depth[fin ^ 1u], 0, (size_t)((D.n + 3u) / 4u)",
                                        "hipMemsetAsync(D.depth[fin ^ 1u], 1, D.n, stream)", "pow_launch_pool_above_subtree(",
                                        "pow_launch_pool_above_count(")]
    assert order == sorted(order)  # whole words to 0 first, then D.n bytes to 1: the last word's tail stays 0
    # the drop: dead from before the keep-marks until the compaction is through, and for good if they kept everything
    order = [drop.index(s) for s in ("ctx->stats = pow_stats{}", "p->dead = true;", "pool_above_run(",
                                     "if (kept >= p->size) return fail(POW_EHIP,", "pool_compact(p, kept, map)",
                                     "p->dead = false;")] + [drop.rindex("return pool_result(p, info);")]
    assert order == sorted(order) and drop.count("return pool_result(p, info);") == 2  # no roots, and the drop's end
    assert drop.count("p->dead = true;") == drop.count("p->dead = false;") == drop.count("pow_stats{}") == 1
    assert "ctx->stats." not in drop  # both sections add into the stats through timed_end: nothing is patched up
    # no state bit hands one call over to another: the compaction has one statement and two callers, nothing inside
    # the library calls the public prune, and the mark's section is only the mark's
    from mpi_blockchain_amd import build
    from test_build import _strip_comments_and_strings
    from test_pool_deep_host import function_bodies
    bodies = function_bodies(_strip_comments_and_strings(open(os.path.join(CSRC, "pow_api.cpp")).read()))
    assert [fn for fn, body in bodies if "pow_queue_pool_compact(" in body] == ["pool_compact"]
    assert [fn for fn, body in bodies if re.search(r"\bpool_compact\(", body)] == ["pow_pool_prune", "pow_pool_drop"]
    for f in build.SOURCES + build.HEADERS:
        text = open(os.path.join(CSRC, f)).read()
        assert "keep_ready" not in text, f
        assert not [fn for fn, body in function_bodies(_strip_comments_and_strings(text)) if "pow_pool_prune(" in body], f
    for dirpath, _, files in os.walk(CSRC):
        for f in files:
            assert "keep_ready" not in open(os.path.join(dirpath, f), errors="replace").read(), f
    mark_run = pool_function("pool_mark_run")
    assert "h_ctl.p->marked" not in mark_run and mark_run.index("const uint32_t n = p->size") < mark_run.index("RESERVE(")
    assert mark_run.count("return POW_OK;") == 1  # one way through


def test_the_hook_runs_the_librarys_sequences():
    hooks = open(os.path.join(CSRC, "pow_hooks.cpp")).read()
    body = hooks[hooks.index('extern "C" int pow_test_pool_above('):]
    for name in QUEUES + ("pow_queue_pool_lift",):
        assert f"{name}(ctx->stream, " in body, name
    # ... and the compaction through the second half it shares with the prune's hook
    half = hooks[hooks.index("int compact_half("):hooks.index("}  // namespace\n\n// The kernels' leading-zero count")]
    assert "pow_queue_pool_compact(ctx->stream, F, T, cap, fin, map != nullptr)" in half and "pow_launch_pool" not in half
    assert body.count("compact_half(f, ") == 1 and hooks.count("compact_half(f, ") == 2
    assert hooks.count("pow_queue_pool_compact(") == 1
    assert "pow_launch_pool" not in body and "hipLaunchKernelGGL" not in hooks
    from mpi_blockchain_amd import build
    assert "pow_hooks.cpp" in build.TEST_ONLY
