"""Codegen and source guards for the batch audit kernel K7
(csrc/pow_verify_batch.hip; CPU only: hipcc cross-compiles gfx950).

K7 keeps K3's budget (pow_node's receive context runs beside K1): at most 64
VGPRs, no scratch, no spills, and the LDS of the 64 + 1 block tile only.  K3
and K7 share one copy of the per-block audit (csrc/pow_audit_dev.h)."""
import os
import re
import subprocess
import tempfile

import pytest

from test_build import CSRC, ROOT, api_function, null_stream_calls, timed_section_helpers

KERNEL = "_Z23pow_verify_batch_kernel"
SRC = "pow_verify_batch.hip"
SHARED = "pow_audit_dev.h"


@pytest.fixture(scope="module")
def isa():
    from mpi_blockchain_amd.build import hipcc

    with tempfile.TemporaryDirectory() as td:
        subprocess.run([hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-mcode-object-version=5",
                        "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-c",
                        os.path.join(CSRC, SRC), "-o", os.path.join(td, "v.o"),
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


def test_batch_verify_kernel_fits_beside_k1(isa):
    md = kernel_metadata(isa)
    assert md["vgpr_count"] <= 64, md
    assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md
    assert md["private_segment_fixed_size"] == 0, md
    assert 65 * 552 <= md["group_segment_fixed_size"] <= 64 * 1024, md  # the 64 + 1 block tile, nothing else
    assert md["wavefront_size"] == 64 and md["max_flat_workgroup_size"] == 64, md


def test_batch_verify_kernel_loads_its_tile_in_16_byte_vectors(isa):
    m = re.search(rf"^({KERNEL}\w*):[^\n]*\n(.*?)s_endpgm", isa, flags=re.S | re.M)
    assert m
    body = m.group(2)
    assert "global_load_dwordx4" in body and re.search(r"ds_write_b128|ds_store_b128", body)
    assert not re.search(r"^\s+scratch_", body, flags=re.M)
    # the verdicts are vector atomics, and only those two
    assert "global_atomic_umin" in body and "global_atomic_add" in body


def test_batch_verify_is_in_both_libraries():
    from mpi_blockchain_amd import build

    for test in (False, True):
        assert os.path.join(CSRC, SRC) in build.sources(test=test)
    assert SHARED in build.HEADERS  # a change of the shared audit rebuilds the libraries


def test_no_null_stream_in_batch_verify_sources():
    found = {}
    for f in (SRC, SHARED, "pow_api.cpp", "pow_ctx.h"):
        hits = null_stream_calls(open(os.path.join(CSRC, f)).read())
        if hits:
            found[f] = hits
    assert not found, found
    # the tiles' copy up and the bounded wait are in the walk the call shares with pow_verify_chain
    body, h = api_function("pow_verify_chains"), timed_section_helpers()
    assert body.count("verify_tiles(") == 1 and "hipMemcpyAsync(" in body and "hipMemsetAsync(" in body
    assert "hipMemcpyAsync(" in h["verify_tiles"]
    union = body + h["verify_tiles"] + h["timed_begin"] + h["timed_end"]
    assert union.count("stream_wait_for(") == 1 and not null_stream_calls(union)
    assert "padded_message" not in union  # no per-block host work
    assert "pow_launch_verify_batch(" in body


def test_one_copy_of_the_audit():
    """K3 and K7 both take the per-block audit from the shared header; neither
    file calls the compression itself, and the header holds the one call."""
    for f in ("pow_verify.hip", SRC):
        text = open(os.path.join(CSRC, f)).read()
        assert f'#include "{SHARED}"' in text, f
        assert "compress(" not in text, f
        assert "audit_block(" in text, f
    shared = open(os.path.join(CSRC, SHARED)).read()
    assert shared.count("compress(h, w)") == 1 and "__forceinline__ uint32_t audit_block(" in shared
