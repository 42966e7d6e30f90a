"""Codegen and source guards for K8, the kernel of pow_mine_rand
(csrc/pow_rand.hip; CPU only: hipcc cross-compiles gfx950).  Metadata and
source checks only."""
import os
import re
import subprocess
import tempfile

import pytest

from mpi_blockchain_amd import _lib

from test_build import CSRC, ROOT, api_function, null_stream_calls, rand_frame_helpers, timed_section_helpers

KERNEL = "_Z15pow_rand_kernel"
SWITCHES = (b"POW_RAND_RUN", b"POW_RAND_LANES_LOG2", b"POW_RAND_LAUNCH_LOG2")
STATE_BYTES = 31 * 256 * 4  # a lane's 31 words, [word][lane]


@pytest.fixture(scope="module")
def metadata():
    from mpi_blockchain_amd.build import hipcc

    with tempfile.TemporaryDirectory() as td:
        subprocess.run([hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-mcode-object-version=5",
                        "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-c",
                        os.path.join(CSRC, "pow_rand.hip"), "-o", os.path.join(td, "r.o"),
                        "-save-temps=obj"], check=True, cwd=td, capture_output=True)
        s = [f for f in os.listdir(td) if f.endswith("gfx950.s")]
        assert s
        isa = open(os.path.join(td, s[0])).read()
    for blk in isa.split("  - .agpr_count")[1:]:
        nm = re.search(r"\.name:\s+(\S+)", blk)
        if nm and nm.group(1).startswith(KERNEL):
            return {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", blk, flags=re.M)}
    raise AssertionError(KERNEL)


def test_rand_kernel_has_no_scratch(metadata):
    md = metadata
    assert md["private_segment_fixed_size"] == 0, md
    assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md
    assert md["vgpr_count"] <= 128, md  # four waves per SIMD, as K4
    assert md["vgpr_count"] <= 125, md  # what it had before the generator moved to pow_rand_dev.h
    assert md["wavefront_size"] == 64 and md["max_flat_workgroup_size"] == 256, md


def test_rand_kernel_lds_fits_four_workgroups_per_cu(metadata):
    # the lanes' states, and the walk's share as K5 counts it: the template, chunk 0 and the four expanded chunks
    lds = metadata["group_segment_fixed_size"]
    assert STATE_BYTES + 552 + 64 + 1024 <= lds <= 40 * 1024, lds
    assert 4 * lds <= 160 * 1024
    assert lds == 33712, lds  # the layout did not move with the generator


def test_rand_kernel_is_in_both_libraries():
    from mpi_blockchain_amd import build

    for test in (False, True):
        assert os.path.join(CSRC, "pow_rand.hip") in build.sources(test=test)
    assert "pow_rand.hip" not in build.TEST_ONLY


def test_no_null_stream_in_rand_sources():
    found = {}
    for f in ("pow_rand.hip", "pow_api.cpp", "pow_ctx.h"):
        hits = null_stream_calls(open(os.path.join(CSRC, f)).read())
        if hits:
            found[f] = hits
    assert not found, found
    # one plain stream launch behind one bounded wait per launch, through the timed section; no graph
    # (the call's timed_end( is rand_timed_end(, the closer it shares with pow_find_seed)
    body, h, shared = api_function("pow_mine_rand"), timed_section_helpers(), rand_frame_helpers()
    union = body + h["timed_begin"] + h["timed_end"]
    assert not null_stream_calls(union)
    assert body.count("pow_launch_rand(ctx->stream") == 1 and body.count("timed_begin(") == 1
    assert body.count("timed_end(") == 1 and union.count("stream_wait_for(") == 1
    assert body.count("rand_timed_end(") == 1 and body.count("stage_rand_tables(") == 1
    assert "hipGraph" not in union + shared and "hipGraph" not in open(os.path.join(CSRC, "pow_rand.hip")).read()
    # the tables go up first, then the launch's input, then the timed section
    order = [body.index(s) for s in ("stage_rand_tables(", "hipMemcpyAsync(D, H,", "timed_begin(", "pow_launch_rand(",
                                     "rand_timed_end(")]
    assert order == sorted(order)
    # the generator and the plan are the HIP-free ones
    host = open(os.path.join(CSRC, "pow_host.cpp")).read()
    for fn in ("pow_rand_plan(", "pow_rand_power(", "pow_rand_apply(", "pow_rand_seed(", "pow_rand_tables("):
        assert fn in body + shared and fn in host, fn
    assert "pow_rand_jumps(" in body
    assert "hip" not in re.sub(r"//[^\n]*", "", host[host.index("void pow_rand_seed"):host.index('extern "C"')]).lower()
    # ... and never libc's
    for f in ("pow_host.cpp", "pow_api.cpp", "pow_rand.hip"):
        src = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, f)).read())
        assert not re.search(r"\bs?rand\s*\(", src), f


def test_rand_buffers_are_released():
    ctxh = open(os.path.join(CSRC, "pow_ctx.h")).read()
    release = ctxh[ctxh.index("void release_buffers()"):]
    release = release[:release.index("}")]
    for name in re.findall(r"^\s+(?:DevBuf|HostBuf)<[^>]+>\s+([^;]+);", ctxh, flags=re.M):
        for n in name.split(","):
            assert f"{n.strip()}.release()" in release, n


def test_rand_kernel_never_waits_for_another_workgroup():
    """No grid barrier and no loop on a word another workgroup writes, in the
    kernel's own file and the shared pow_walk_dev.h: the same check K4-K6 have.
    pow_rand_dev.h, the generator it shares with K9, shares no word at all."""
    own = open(os.path.join(CSRC, "pow_rand.hip")).read()
    gen = open(os.path.join(CSRC, "pow_rand_dev.h")).read()
    src = own + open(os.path.join(CSRC, "pow_walk_dev.h")).read() + gen
    assert '#include "pow_rand_dev.h"' in own
    gen_code = re.sub(r"//[^\n]*", "", gen)
    for word in ("load_agent", "volatile", "__threadfence", "atomic", "cooperative_groups", "grid.sync"):
        assert word not in gen_code, word
    assert "cooperative_groups" not in src and "grid.sync" not in src
    loops = re.findall(r"\b(?:while|for)\s*\(([^\n]*)\)\s*\{?\s*$", src, flags=re.M)
    assert loops
    for cond in loops:
        for word in ("exits", "stop", "left", "seen", "min_rel", "min_key", "n_done", "slots"):
            assert word not in cond, cond
    # K8's one walk loop is its own, on a lane-local flag
    assert len(re.findall(r"\bwhile\s*\(", own)) == 1 and re.search(r"\bwhile \(go\) \{", own)
    # and it shares the rest with K4-K6
    for shared in ("expand(", "trial_of(", "leave(", "winner("):
        assert shared in own, shared


def test_the_generator_is_on_the_device_once():
    """K9 began as a copy of K8's generator.  The polynomial's multiply-add
    loop, the workgroup's move and the layout of the runs live in
    pow_rand_dev.h; neither kernel file restates them."""
    files = {f: re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, f)).read())
             for f in ("pow_rand.hip", "pow_seed.hip", "pow_rand_dev.h")}
    loop = re.compile(r"#pragma unroll 1\s+for \([^\n]*\) \{\s+const uint32_t c = coef\(i\);")
    for pattern in (loop, re.compile(r"y\[j\] \+= c \* x\[j\]"), re.compile(r"\bvoid group_move\("),
                    re.compile(r"xe\[k - NW\] \+ xe\[k - 3u\]"), re.compile(r"nwg \* \w+ \* run - run")):
        assert {f: len(pattern.findall(s)) for f, s in files.items()} == \
            {"pow_rand.hip": 0, "pow_seed.hip": 0, "pow_rand_dev.h": 1}, pattern.pattern
    for f in ("pow_rand.hip", "pow_seed.hip"):
        assert '#include "pow_rand_dev.h"' in files[f], f
        assert not re.search(r"constexpr uint32_t (NW|WG)\b", files[f]), f
        assert "256" not in re.sub(r"__launch_bounds__\(256\)", "", files[f]), f  # the table layout's stride is the header's
    assert "pow_walk_dev.h" not in files["pow_seed.hip"] and "pow_walk_dev.h" not in files["pow_rand_dev.h"]


def test_switches_only_in_the_test_library():
    shipped = open(_lib.LIB_PATH, "rb").read()
    test = open(_lib.TEST_LIB_PATH, "rb").read()
    assert [s for s in SWITCHES if s in shipped] == []
    assert all(s in test for s in SWITCHES)
    hooks = open(os.path.join(CSRC, "pow_hooks.cpp")).read()
    for f in os.listdir(CSRC):
        p = os.path.join(CSRC, f)
        if os.path.isfile(p) and f != "pow_hooks.cpp":
            assert 'getenv("POW_RAND' not in open(p).read(), f
    for s in SWITCHES:
        assert f'getenv("{s.decode()}")' in hooks
