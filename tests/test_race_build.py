"""Codegen and source guards for the race kernel K6 (csrc/pow_race.hip; CPU
only: hipcc cross-compiles gfx950)."""
import os
import re
import subprocess
import tempfile

import pytest

from mpi_blockchain_amd import _lib

from test_build import CSRC, ROOT, api_function, null_stream_calls, timed_section_helpers

KERNEL = "_Z15pow_race_kernel"
SWITCHES = (b"POW_RACE_FUSED_MAX", b"POW_RACE_BATCH", b"POW_RACE_LANES_LOG2")


@pytest.fixture(scope="module")
def isa():
    from mpi_blockchain_amd.build import hipcc

    with tempfile.TemporaryDirectory() as td:
        subprocess.run([hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-mcode-object-version=5",
                        "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-c",
                        os.path.join(CSRC, "pow_race.hip"), "-o", os.path.join(td, "r.o"),
                        "-save-temps=obj"], check=True, cwd=td, capture_output=True)
        s = [f for f in os.listdir(td) if f.endswith("gfx950.s")]
        assert s
        return open(os.path.join(td, s[0])).read()


def kernel_metadata(isa: str) -> dict:
    for blk in isa.split("  - .agpr_count")[1:]:
        nm = re.search(r"\.name:\s+(\S+)", blk)
        if nm and nm.group(1).startswith(KERNEL):
            return {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", blk, flags=re.M)}
    raise AssertionError(KERNEL)


def test_race_kernel_has_no_scratch(isa):
    md = kernel_metadata(isa)
    assert md["private_segment_fixed_size"] == 0, md
    assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md
    # four waves per SIMD, as K4
    assert md["vgpr_count"] <= 128, md
    assert md["wavefront_size"] == 64 and md["max_flat_workgroup_size"] == 256, md
    # the parent, the sealed block, chunk 0 and the four expanded chunks, and a few words: nowhere near a CU's LDS
    assert 2 * 552 + 64 + 1024 <= md["group_segment_fixed_size"] <= 4096, md
    m = re.search(rf"^({KERNEL}\w*):[^\n]*\n(.*?)s_endpgm", isa, flags=re.S | re.M)
    assert m and not re.search(r"^\s+scratch_", m.group(2), flags=re.M)


def test_race_kernel_is_in_both_libraries():
    from mpi_blockchain_amd import build

    for test in (False, True):
        assert os.path.join(CSRC, "pow_race.hip") in build.sources(test=test)


def test_no_null_stream_in_race_sources():
    found = {}
    for f in ("pow_race.hip", "pow_api.cpp", "pow_ctx.h"):
        hits = null_stream_calls(open(os.path.join(CSRC, f)).read())
        if hits:
            found[f] = hits
    assert not found, found
    # the batch's bounded wait is in the timed section's closer, the host loop in the one shared with pow_mine_chain
    body, h, host = api_function("pow_mine_race"), timed_section_helpers(), api_function("mine_linked_host")
    union = body + h["timed_begin"] + h["timed_end"] + host
    assert not null_stream_calls(union)
    # plain stream launches behind one bounded wait and one copy back per batch; no graph
    assert body.count("pow_launch_race(ctx->stream") == 1 and body.count("timed_end(") == 1
    assert union.count("stream_wait_for(") == 1
    assert union.count("hipMemcpyDeviceToHost") == 1
    assert "hipGraph" not in union and "hipGraph" not in open(os.path.join(CSRC, "pow_race.hip")).read()
    # one rival is pow_mine_chain, and the host loop is pow_mine's own implementation under the best counter so far
    assert "return rc;" in body and "pow_mine_chain(ctx, parent, n, diff_bits" in body
    assert body.count("mine_linked_host(") == 1 and "mine_impl(ctx, &tmpl, ctr_start, window" in host
    # the plan is the HIP-free one
    assert "pow_race_plan(" in body and "pow_race_plan(" in open(os.path.join(CSRC, "pow_host.cpp")).read()


def test_race_kernel_never_waits_for_another_workgroup():
    """No grid barrier and no loop on a word another workgroup writes: the only
    loops of the kernel (its own file and the shared pow_walk_dev.h) are the
    lane's walk of its counters, the chunk and schedule loops, the last
    workgroup's strided pass over the slots and its pass over the block's bytes."""
    src = open(os.path.join(CSRC, "pow_race.hip")).read() + open(os.path.join(CSRC, "pow_walk_dev.h")).read()
    assert "cooperative_groups" not in src and "grid.sync" not in src
    loops = re.findall(r"\b(?:while|for)\s*\(([^\n]*)\)\s*\{?\s*$", src, flags=re.M)
    assert loops
    for cond in loops:
        for word in ("exits", "stop", "left", "seen", "min_key", "n_done", "slots"):
            assert word not in cond, cond
    # the walk's own condition is a lane-local flag
    assert re.search(r"\bwhile \(go\) \{", src) and len(re.findall(r"\bwhile\b\s*\(", src)) == 1


def test_switches_only_in_the_test_library():
    shipped = open(_lib.LIB_PATH, "rb").read()
    test = open(_lib.TEST_LIB_PATH, "rb").read()
    assert [s for s in SWITCHES if s in shipped] == []
    assert all(s in test for s in SWITCHES)
    hooks = open(os.path.join(CSRC, "pow_hooks.cpp")).read()
    for f in os.listdir(CSRC):
        p = os.path.join(CSRC, f)
        if os.path.isfile(p) and f != "pow_hooks.cpp":
            assert 'getenv("POW_RACE' not in open(p).read(), f
    for s in SWITCHES:
        assert f'getenv("{s.decode()}")' in hooks


def test_fused_threshold_is_within_the_kernel_s_range():
    ctxh = open(os.path.join(CSRC, "pow_ctx.h")).read()
    m = re.search(r"^#define POW_RACE_FUSED_MAX_D\s+\(?(-?\d+)\)?\s*$", ctxh, flags=re.M)
    assert m and -1 <= int(m.group(1)) <= 32  # K6 tests H0 <= thr: 32 bits at most
    # a key carries the rival in 8 bits, and the header's limit is that
    hdr = open(os.path.join(ROOT, "include", "pow_gpu.h")).read()
    assert re.search(r"^#define POW_RACE_MAX_RIVALS 256\s*$", hdr, flags=re.M)
