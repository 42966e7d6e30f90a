"""Codegen and source guards for K9, the kernel of pow_find_seed
(csrc/pow_seed.hip; CPU only: hipcc cross-compiles gfx950).  Metadata and
source checks only."""
import os
import re
import subprocess
import tempfile

import pytest

from mpi_blockchain_amd import _lib

from test_build import CSRC, ROOT, api_function, null_stream_calls, rand_frame_helpers, timed_section_helpers

KERNEL = "_Z15pow_seed_kernel"
SWITCHES = (b"POW_SEED_RUN", b"POW_SEED_WG", b"POW_SEED_LAUNCH_LOG2")


@pytest.fixture(scope="module")
def isa():
    from mpi_blockchain_amd.build import hipcc

    with tempfile.TemporaryDirectory() as td:
        subprocess.run([hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-mcode-object-version=5",
                        "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-c",
                        os.path.join(CSRC, "pow_seed.hip"), "-o", os.path.join(td, "s.o"),
                        "-save-temps=obj"], check=True, cwd=td, capture_output=True)
        s = [f for f in os.listdir(td) if f.endswith("gfx950.s")]
        assert s
        return open(os.path.join(td, s[0])).read()


@pytest.fixture(scope="module")
def metadata(isa):
    for blk in isa.split("  - .agpr_count")[1:]:
        nm = re.search(r"\.name:\s+(\S+)", blk)
        if nm and nm.group(1).startswith(KERNEL):
            return {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", blk, flags=re.M)}
    raise AssertionError(KERNEL)


def test_seed_kernel_has_no_scratch(metadata):
    """The 31-word state is registers: a register array indexed dynamically
    would live in scratch, and show here."""
    md = metadata
    assert md["private_segment_fixed_size"] == 0, md
    assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md
    assert md["vgpr_count"] <= 128, md  # where it stood before the generator moved to pow_rand_dev.h, too
    assert md["wavefront_size"] == 64 and md["max_flat_workgroup_size"] == 256, md


def test_seed_kernel_touches_no_scratch_memory(isa):
    body = isa[isa.index(KERNEL):]
    assert not re.search(r"^\s*(scratch_|buffer_(load|store))", body, flags=re.M)


def test_seed_kernel_state_is_not_in_lds(metadata):
    # the register form: the workgroup's 62 words, the 62 x 62-bit table and 64 targets; no lane's state
    lds = metadata["group_segment_fixed_size"]
    assert 62 * 8 + 64 * 8 <= lds < 4 * 1024, lds
    assert lds < 31 * 256 * 4
    assert lds == 1760, lds  # the layout did not move with the generator


def test_seed_kernel_is_in_both_libraries():
    from mpi_blockchain_amd import build

    for test in (False, True):
        assert os.path.join(CSRC, "pow_seed.hip") in build.sources(test=test)
    assert "pow_seed.hip" not in build.TEST_ONLY
    for path in (_lib.LIB_PATH, _lib.TEST_LIB_PATH):
        assert KERNEL.encode() in open(path, "rb").read(), path


def test_no_null_stream_in_seed_sources():
    found = {}
    for f in ("pow_seed.hip", "pow_api.cpp", "pow_ctx.h"):
        hits = null_stream_calls(open(os.path.join(CSRC, f)).read())
        if hits:
            found[f] = hits
    assert not found, found
    # one plain stream launch behind one bounded wait per launch, through the timed section; no graph
    # (the call's timed_end( is rand_timed_end(, the closer it shares with pow_mine_rand)
    body, h, shared = api_function("pow_find_seed"), timed_section_helpers(), rand_frame_helpers()
    union = body + h["timed_begin"] + h["timed_end"]
    assert not null_stream_calls(union)
    assert body.count("pow_launch_seed(ctx->stream") == 1 and body.count("timed_begin(") == 1
    assert body.count("timed_end(") == 1 and union.count("stream_wait_for(") == 1
    assert body.count("rand_timed_end(") == 1 and body.count("stage_rand_tables(") == 1
    kernel = open(os.path.join(CSRC, "pow_seed.hip")).read()
    assert "hipGraph" not in union + shared and "hipGraph" not in kernel
    assert kernel.count("hipLaunchKernelGGL(pow_seed_kernel") == 1 and "<<<" not in kernel
    # the tables go up first, then the launch's input, then the timed section
    order = [body.index(s) for s in ("stage_rand_tables(", "hipMemcpyAsync(ctx->d_seed.p, H,", "timed_begin(",
                                     "pow_launch_seed(", "rand_timed_end(")]
    assert order == sorted(order)
    # the generator, the plan and the packing are the HIP-free ones
    host = open(os.path.join(CSRC, "pow_host.cpp")).read()
    for fn in ("pow_seed_plan(", "pow_seed_pack(", "pow_rand_power(", "pow_rand_mul(", "pow_rand_tables("):
        assert fn in body + shared and fn in host, fn
    assert "pow_rand_jumps(" in body
    assert "hip" not in re.sub(r"//[^\n]*", "", host[host.index("bool pow_seed_pack"):host.index('extern "C"')]).lower()
    # there is no per-seed host work: the host's seeding is not called
    assert "pow_rand_seed(" not in body


def test_no_libc_generator_in_the_sources():
    for f in ("pow_host.cpp", "pow_api.cpp", "pow_seed.hip", "pow_hooks.cpp"):
        src = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, f)).read())
        assert not re.search(r"\bs?rand\s*\(", src), f
    example = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "examples", "find_seed.c")).read(), flags=re.S)
    assert not re.search(r"\bs?rand\s*\(", example)


def test_seed_kernel_never_waits_for_another_workgroup():
    """No grid barrier and no loop on a word another workgroup writes: the only
    word the workgroups share is the match counter, and nobody reads it but
    through the atomic add that reserves a slot.  The generator's header,
    which the kernel's file includes, is read with it: it has no atomic at all."""
    own = open(os.path.join(CSRC, "pow_seed.hip")).read()
    gen = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "pow_rand_dev.h")).read())
    assert '#include "pow_rand_dev.h"' in own and re.findall(r'#include "([^"]+)"', gen) == ["pow_ctx.h"]
    assert "atomic" not in gen
    code = re.sub(r"//[^\n]*", "", own) + gen
    assert "cooperative_groups" not in code and "grid.sync" not in code and "pow_walk_dev.h" not in code
    loops = re.findall(r"\b(?:while|for)\s*\(([^\n]*)\)\s*\{?\s*$", code, flags=re.M)
    assert loops
    for cond in loops:
        for word in ("out", "->n", "exits", "stop", "seen", "load_agent", "volatile", "atomic"):
            assert word not in cond, cond
    assert len(re.findall(r"\bwhile\s*\(", code)) == 1 and re.search(r"\bwhile \(rel < L\.count\) \{", code)
    assert "load_agent" not in code and "volatile" not in code and "__threadfence" not in code
    assert len(re.findall(r"\batomic\w+\(", code)) == 1 and "atomicAdd(&out->n, 1u)" in code
    # every store to the list is bounded by its capacity
    assert re.search(r"if \(slot < POW_SEED_DEV_CAP\) \{[^}]*out->rec\[slot\]", code, flags=re.S)
    assert len(re.findall(r"out->rec\[", code)) == 3


def test_switches_only_in_the_test_library():
    shipped = open(_lib.LIB_PATH, "rb").read()
    test = open(_lib.TEST_LIB_PATH, "rb").read()
    assert [s for s in SWITCHES if s in shipped] == []
    assert all(s in test for s in SWITCHES)
    hooks = open(os.path.join(CSRC, "pow_hooks.cpp")).read()
    for f in os.listdir(CSRC):
        p = os.path.join(CSRC, f)
        if os.path.isfile(p) and f != "pow_hooks.cpp":
            assert 'getenv("POW_SEED' not in open(p).read(), f
    for s in SWITCHES:
        assert f'getenv("{s.decode()}")' in hooks


def test_warmup_does_not_launch_the_kernel():
    assert "pow_launch_seed" not in api_function("pow_warmup")
