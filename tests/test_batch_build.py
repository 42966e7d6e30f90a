"""Codegen and source guards for the batch-mining kernel K5
(csrc/pow_batch.hip; CPU only: hipcc cross-compiles gfx950)."""
import os
import re
import subprocess
import tempfile

import pytest

from mpi_blockchain_amd import _lib

from test_build import CSRC, ROOT, api_function, null_stream_calls, timed_section_helpers

KERNEL = "_Z16pow_batch_kernel"
SWITCHES = (b"POW_BATCH_FUSED_MAX", b"POW_BATCH_TILE", b"POW_BATCH_LANES_LOG2")


@pytest.fixture(scope="module")
def isa():
    from mpi_blockchain_amd.build import hipcc

    with tempfile.TemporaryDirectory() as td:
        subprocess.run([hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-mcode-object-version=5",
                        "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-c",
                        os.path.join(CSRC, "pow_batch.hip"), "-o", os.path.join(td, "b.o"),
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


def test_batch_kernel_has_no_scratch(isa):
    md = kernel_metadata(isa)
    assert md["private_segment_fixed_size"] == 0, md
    assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md
    # four waves per SIMD, as K4
    assert md["vgpr_count"] <= 128, md
    assert md["wavefront_size"] == 64 and md["max_flat_workgroup_size"] == 256, md
    # the template, chunk 0 and the four expanded chunks, and a few words: nowhere near a CU's LDS
    assert 552 + 64 + 1024 <= md["group_segment_fixed_size"] <= 4096, md
    m = re.search(rf"^({KERNEL}\w*):[^\n]*\n(.*?)s_endpgm", isa, flags=re.S | re.M)
    assert m and not re.search(r"^\s+scratch_", m.group(2), flags=re.M)


def test_batch_kernel_is_in_both_libraries():
    from mpi_blockchain_amd import build

    for test in (False, True):
        assert os.path.join(CSRC, "pow_batch.hip") in build.sources(test=test)


def test_no_null_stream_in_batch_sources():
    found = {}
    for f in ("pow_batch.hip", "pow_api.cpp", "pow_ctx.h"):
        hits = null_stream_calls(open(os.path.join(CSRC, f)).read())
        if hits:
            found[f] = hits
    assert not found, found
    # the tile's bounded wait is in the timed section's closer
    body, h = api_function("pow_mine_batch"), timed_section_helpers()
    union = body + h["timed_begin"] + h["timed_end"]
    assert not null_stream_calls(union)
    # one plain stream launch behind one bounded wait per tile; no graph
    assert body.count("pow_launch_batch(ctx->stream") == 1 and body.count("timed_end(") == 1
    assert union.count("stream_wait_for(") == 1
    assert "hipGraph" not in union and "hipGraph" not in open(os.path.join(CSRC, "pow_batch.hip")).read()
    # n == 1 and the host loop are pow_mine's own implementation
    assert "mine_impl(ctx, &tmpls[i]" in body
    # the plan is the HIP-free one
    assert "pow_batch_plan(" in body and "pow_batch_plan(" in open(os.path.join(CSRC, "pow_host.cpp")).read()


def test_batch_kernel_never_waits_for_another_workgroup():
    """No grid barrier and no loop on a word another workgroup writes: the only
    loops of the kernel (its own file and the shared pow_walk_dev.h) are the
    lane's walk of its counters, the chunk and schedule loops and the last
    workgroup's strided pass over the slots."""
    src = open(os.path.join(CSRC, "pow_batch.hip")).read() + open(os.path.join(CSRC, "pow_walk_dev.h")).read()
    assert "cooperative_groups" not in src and "grid.sync" not in src
    loops = re.findall(r"\b(?:while|for)\s*\(([^\n]*)\)\s*\{?\s*$", src, flags=re.M)
    assert loops
    for cond in loops:
        for word in ("exits", "stop", "left", "seen", "min_rel", "min_key", "n_done", "slots"):
            assert word not in cond, cond
    # the walk's own condition is a lane-local flag
    assert re.search(r"\bwhile \(go\) \{", src)


def test_switches_only_in_the_test_library():
    shipped = open(_lib.LIB_PATH, "rb").read()
    test = open(_lib.TEST_LIB_PATH, "rb").read()
    assert [s for s in SWITCHES if s in shipped] == []
    assert all(s in test for s in SWITCHES)
    hooks = open(os.path.join(CSRC, "pow_hooks.cpp")).read()
    for f in os.listdir(CSRC):
        p = os.path.join(CSRC, f)
        if os.path.isfile(p) and f != "pow_hooks.cpp":
            assert 'getenv("POW_BATCH' not in open(p).read(), f
    for s in SWITCHES:
        assert f'getenv("{s.decode()}")' in hooks


def test_fused_threshold_is_within_the_kernel_s_range():
    ctxh = open(os.path.join(CSRC, "pow_ctx.h")).read()
    m = re.search(r"^#define POW_BATCH_FUSED_MAX_D\s+\(?(-?\d+)\)?\s*$", ctxh, flags=re.M)
    assert m and -1 <= int(m.group(1)) <= 32  # K5 tests H0 <= thr: 32 bits at most
