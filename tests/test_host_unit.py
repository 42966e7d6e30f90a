"""The HIP-free host code (csrc/pow_host.cpp: template precompute, K2' message
schedules, launch splitting, nonce / serializer / difficulty helpers) on the
CPU under AddressSanitizer + UndefinedBehaviorSanitizer.

tests/host_unit.cpp links pow_host.cpp alone and runs as a process of its own:
nothing is loaded into Python.  It gets the golden templates, digests and
random blocks as text lines on stdin.  CPU only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpi_blockchain_amd", "csrc")


def golden_lines(golden) -> str:
    out = []
    for t in golden["templates"]:
        out.append(f"T {t['name']} {t['index']} {t['node_owner_number']} {t['difficulty']} {t['created_at']} "
                   f"{t['previous_block_hash_hex']}")
    for e in golden["digests"]:
        out.append(f"D {e['template']} {e['counter']} {e['hex']} {int(e['solves_d9'])}")
    for e in golden["random_blocks"]:
        out.append(f"R {e['index']} {e['node_owner_number']} {e['difficulty']} {e['created_at']} {e['nonce_hex']} "
                   f"{e['previous_block_hash_hex']} {e['hex']}")
    return "\n".join(out) + "\n"


def test_host_code_under_sanitizers(golden, tmp_path):
    assert (len(golden["templates"]), len(golden["digests"]), len(golden["random_blocks"])) == (4, 96, 48)
    exe = str(tmp_path / "host_unit")
    # no ROCm include path: pow_host.cpp and its headers are HIP-free
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "host_unit.cpp"), os.path.join(CSRC, "pow_host.cpp"), "-o", exe],
                   check=True, cwd=str(tmp_path))
    r = subprocess.run([exe], input=golden_lines(golden), capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "4 templates, 96 digests, 48 random blocks" in r.stdout and " 0 failed" in r.stdout, r.stdout
