"""Codegen and source guards for the chain-verification kernel K3
(csrc/pow_verify.hip; CPU only: hipcc cross-compiles gfx950).

pow_node runs K3 on its receive context while K1 fills all but one workgroup
slot of every CU, so K3 keeps K2's budget: at most 64 VGPRs, no scratch, no
spills; and its LDS tile (64 blocks + 1 halo block) must leave room beside
K1's."""
import os
import re
import subprocess
import tempfile

import pytest

from test_build import CSRC, ROOT, api_function, null_stream_calls, timed_section_helpers

KERNEL = "_Z17pow_verify_kernel"


@pytest.fixture(scope="module")
def isa():
    from mpi_blockchain_amd.build import hipcc

    with tempfile.TemporaryDirectory() as td:
        subprocess.run([hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-mcode-object-version=5",
                        "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-c",
                        os.path.join(CSRC, "pow_verify.hip"), "-o", os.path.join(td, "v.o"),
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


def test_verify_kernel_fits_beside_k1(isa):
    md = kernel_metadata(isa)
    assert md["vgpr_count"] <= 64, md
    assert md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0, md
    assert md["private_segment_fixed_size"] == 0, md
    assert 65 * 552 <= md["group_segment_fixed_size"] <= 64 * 1024, md  # the 64 + 1 block tile, nothing else
    assert md["wavefront_size"] == 64 and md["max_flat_workgroup_size"] == 64, md


def test_verify_kernel_loads_its_tile_in_16_byte_vectors(isa):
    m = re.search(rf"^({KERNEL}\w*):[^\n]*\n(.*?)s_endpgm", isa, flags=re.S | re.M)
    assert m
    body = m.group(2)
    assert "global_load_dwordx4" in body and re.search(r"ds_write_b128|ds_store_b128", body)
    assert not re.search(r"^\s+scratch_", body, flags=re.M)


def test_verify_is_in_both_libraries():
    from mpi_blockchain_amd import build

    for test in (False, True):
        assert os.path.join(CSRC, "pow_verify.hip") in build.sources(test=test)


def test_no_null_stream_in_verify_sources():
    """test_build's guard has a fixed file list that does not know
    pow_verify.hip; the same check over it and over pow_api.cpp, which gained
    pow_verify_chain's copies, events and wait."""
    found = {}
    for f in ("pow_verify.hip", "pow_api.cpp", "pow_ctx.h"):
        hits = null_stream_calls(open(os.path.join(CSRC, f)).read())
        if hits:
            found[f] = hits
    assert not found, found
    # the tiles' copy up and the bounded wait are in the walk the call shares with pow_verify_chains
    body, h = api_function("pow_verify_chain"), timed_section_helpers()
    assert body.count("verify_tiles(") == 1 and "hipMemcpyAsync(" in body and "hipMemcpyAsync(" in h["verify_tiles"]
    union = body + h["verify_tiles"] + h["timed_begin"] + h["timed_end"]
    assert union.count("stream_wait_for(") == 1 and not null_stream_calls(union)
    assert "pow_launch_verify(" in body
    assert "padded_message" not in union  # no per-block host work
