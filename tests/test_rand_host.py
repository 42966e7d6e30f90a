"""pow_rand_nonces, the reference's nonce stream on the host, and the argument
checks of pow_mine_rand (CPU only).  The stream is pinned three ways: to libc's
own srand/rand through ctypes, to the pure-Python restatement tests/rand_util.py
and to what the reference's gen_random_nonce gave (tests/golden/rand_replay.json,
and the live reference build where it exists).  K8's plan, its tables and its
lane walk run in tests/rand_plan_unit.cpp, a process of its own under sanitizers."""
import ctypes
import ctypes.util
import json
import os
import subprocess

import pytest

import rand_util
from mpi_blockchain_amd import _lib
from mpi_blockchain_amd.block import make_block
from mpi_blockchain_amd.miner import rand_nonces

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (0, 1, 0x80000000, 0xFFFFFFFF, 1700000003)
LIMIT = 1 << 56


@pytest.fixture(scope="module")
def replay():
    with open(os.path.join(ROOT, "tests", "golden", "rand_replay.json")) as f:
        return json.load(f)


def lib_nonces(seed: int, start: int, n: int) -> bytes:
    buf = ctypes.create_string_buffer(n * 10)
    assert _lib.load().pow_rand_nonces(seed, start, n, buf) == _lib.POW_OK
    return buf.raw


def test_both_names_are_exported():
    assert "pow_rand_nonces" in _lib.EXPORTS and "pow_mine_rand" in _lib.EXPORTS
    L = _lib.load()
    assert L.pow_rand_nonces and L.pow_mine_rand
    assert _lib.RAND_TRIAL_LIMIT == LIMIT


@pytest.mark.parametrize("seed", SEEDS)
def test_equals_libc_rand_over_2p20_trials(seed):
    """9 x rand() % 62 per trial of libc's own generator after srand(seed)."""
    libc = ctypes.CDLL(ctypes.util.find_library("c") or "libc.so.6")
    libc.srand.argtypes = [ctypes.c_uint]
    libc.rand.restype = ctypes.c_int
    n = 1 << 20
    libc.srand(seed)
    rand = libc.rand
    alphabet = rand_util.ALPHABET
    want = bytearray(n * 10)
    for t in range(n):
        o = 10 * t
        for i in range(9):
            want[o + i] = alphabet[rand() % 62]
    got = lib_nonces(seed, 0, n)
    assert got == bytes(want)


def test_seed_zero_is_seed_one():
    assert lib_nonces(0, 0, 4096) == lib_nonces(1, 0, 4096)
    assert lib_nonces(0, 0, 16) != lib_nonces(2, 0, 16)


@pytest.mark.parametrize("start", [0, 1, (1 << 20) + 7, (1 << 40) + 123, LIMIT - 64])
@pytest.mark.parametrize("seed", [1, 0x80000000, 1700000003])
def test_equals_the_restatement_after_a_jump(seed, start):
    n = 64  # LIMIT - 64: up to the limit itself
    assert lib_nonces(seed, start, n) == b"".join(rand_util.nonces(seed, start, n))


def test_composition():
    """The nonces at a + b are the same whichever way one gets there."""
    seed, a, b = 12345, (1 << 33) + 5, 777
    walk = lib_nonces(seed, a, b + 8)
    assert walk[10 * b:] == lib_nonces(seed, a + b, 8)
    assert lib_nonces(seed, 0, 300)[10 * 279:] == lib_nonces(seed, 279, 21)
    # ... and in the restatement: x^a x^b = x^(a + b)
    assert rand_util.poly_mul(rand_util.x_power(9 * a), rand_util.x_power(9 * b)) == rand_util.x_power(9 * (a + b))


def test_equals_the_reference_s_recorded_nonces(replay):
    for seed, want in replay["nonces"].items():
        assert [n.hex() for n in rand_nonces(int(seed), 0, len(want))] == want
    # the nonce of every recorded block is the stream's at the recorded trial
    for r in replay["replays"]:
        for b in r["blocks"]:
            assert rand_nonces(r["seed"], b["trial"], 1)[0] == bytes.fromhex(b["block_hex"])[24:34]


def test_equals_the_live_reference_where_it_is_built():
    from oracle.oracle import RefLib, ref_available

    if not ref_available():
        pytest.skip("oracle/_ref is not built")
    R = RefLib("O2")
    for seed in SEEDS:
        R.L.ref_srand(seed)
        want = b"".join(bytes(R.gen_random_nonce()) for _ in range(5000))
        assert lib_nonces(seed, 0, 5000) == want


def test_restated_brute_force_reproduces_the_recorded_replays(replay):
    """tests/rand_util.py's miner, the GPU tests' yardstick, against the reference's own blocks."""
    for r in replay["replays"]:
        last, at = bytes.fromhex(r["parent_hex"]), 0
        for k, b in enumerate(r["blocks"]):
            t = bytearray(last)
            t[0:4] = ((int.from_bytes(last[0:4], "little") + 1) & 0xFFFFFFFF).to_bytes(4, "little")
            t[4:8] = r["rank"].to_bytes(4, "little")
            t[8:12] = r["difficulty"].to_bytes(4, "little")
            t[16:24] = r["created_at"][k].to_bytes(8, "little")
            t[34:290] = last[290:546]
            (trial, nonce, hexd), = rand_util.mine(bytes(t), r["seed"], at, 1 << 20, r["difficulty"])
            assert trial == b["trial"]
            last, at = rand_util.seal(bytes(t), nonce, hexd), trial + 1
            assert last.hex() == b["block_hex"]
        assert at == r["total_trials"]


def test_plan_tables_and_lane_walk_under_sanitizers(tmp_path):
    """tests/rand_plan_unit.cpp links pow_host.cpp alone and runs as a process
    of its own under ASan + UBSan: nothing is loaded into Python."""
    csrc = os.path.join(ROOT, "mpi_blockchain_amd", "csrc")
    exe = str(tmp_path / "rand_plan_unit")
    # no ROCm include path: pow_host.cpp and its headers are HIP-free
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                    os.path.join(ROOT, "tests", "rand_plan_unit.cpp"), os.path.join(csrc, "pow_host.cpp"), "-o", exe],
                   check=True, cwd=str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert " checks, 0 failed" in r.stdout, r.stdout
    assert int(r.stdout.split(" checks, 0 failed")[0].split()[-1]) > 1_000_000  # the sweep ran


def test_seam_fixture_is_hashlib_s(golden):
    """tests/golden/rand_seam.json (gen_rand_seam.py: the GPU only searched) row
    by row: the nonce of the trial, its digest, its leading zero bits, one
    witness on either side of the 32-bit seam, and nothing else near 2^-29 in
    the 2,048-trial window the GPU tests run around it."""
    import hashlib

    with open(os.path.join(ROOT, "tests", "golden", "rand_seam.json")) as f:
        v = json.load(f)
    assert (v["before"], v["window"]) == (1000, 2048)
    rows = v["witnesses"]
    assert [r["leading_zeros"] == 31 for r in rows] == [True, False] and rows[1]["leading_zeros"] >= 32
    templates = {t["name"]: t for t in golden["templates"]}
    for r in rows:
        t = templates[r["template"]]
        assert (r["template"], r["seed"]) == ("S0", 1700000003) and v["before"] <= r["trial"] < LIMIT
        tb = bytes(make_block(t["index"], t["node_owner_number"], t["difficulty"], t["created_at"],
                              bytes.fromhex(t["previous_block_hash_hex"])))
        nonce, = rand_util.nonces(r["seed"], r["trial"], 1)
        assert nonce == r["nonce"].encode() + b"\0" and lib_nonces(r["seed"], r["trial"], 1) == nonce
        digest = hashlib.sha256(rand_util.message(tb, nonce)).digest()
        assert digest.hex() == r["digest"]
        assert 256 - int.from_bytes(digest, "big").bit_length() == r["leading_zeros"]
        assert int.from_bytes(digest[:4], "big") == (1 if r["leading_zeros"] == 31 else 0)  # H0 == thr
        near = rand_util.mine(tb, r["seed"], r["trial"] - v["before"], v["window"], 29, want=v["window"])
        assert near == [(r["trial"], nonce, r["digest"])]


def test_all_62_characters_occur():
    seen = set(lib_nonces(7, 0, 4096)) - {0}
    assert seen == set(rand_util.ALPHABET)
    raw = lib_nonces(7, 0, 4096)
    assert all(raw[10 * t + 9] == 0 for t in range(4096))


def test_rand_nonces_einval_writes_nothing():
    L = _lib.load()
    buf = ctypes.create_string_buffer(b"\xAA" * 40, 40)
    for start, n in ((LIMIT, 1), (LIMIT - 3, 4), (LIMIT + 1, 0), ((1 << 64) - 1, 2)):
        assert L.pow_rand_nonces(1, start, n, buf) == _lib.POW_EINVAL
        assert L.pow_last_error()
        assert buf.raw == b"\xAA" * 40
    assert L.pow_rand_nonces(1, 0, 1, None) == _lib.POW_EINVAL
    # the last trial below the limit, and an empty request at it
    assert L.pow_rand_nonces(1, LIMIT - 1, 1, buf) == _lib.POW_OK and buf.raw[10:] == b"\xAA" * 30
    assert L.pow_rand_nonces(1, LIMIT, 0, None) == _lib.POW_OK
    with pytest.raises(_lib.PowError):
        rand_nonces(1, LIMIT, 1)


def test_mine_rand_einval_in_the_stated_order():
    """diff_bits, then trial_count, then the trial range, then the null
    pointers: each case has every LATER fault too (a null ctx throughout), and
    the message names the first.  Nothing is written."""
    L = _lib.load()
    tmpl = make_block(1, 0, 9, 1700000000)
    out = _lib.Block()
    before = bytes(out)
    found, hashes = ctypes.c_uint64(0x1111), ctypes.c_uint64(0x2222)

    def call(ctx, t, start, count, d, o):
        rc = L.pow_mine_rand(ctx, t, 1, start, count, d, None, 0, o, ctypes.byref(found), ctypes.byref(hashes))
        return rc, (L.pow_last_error() or b"").decode()

    rc, msg = call(None, None, LIMIT, 0, 33, None)
    assert rc == _lib.POW_EINVAL and "diff_bits" in msg
    for count in (0, (1 << 32) + 1):
        rc, msg = call(None, None, LIMIT, count, 32, None)
        assert rc == _lib.POW_EINVAL and "trial_count" in msg
    for start, count in ((LIMIT, 1), (LIMIT - (1 << 32) + 1, 1 << 32), ((1 << 64) - 1, 1)):
        rc, msg = call(None, None, start, count, 9, None)
        assert rc == _lib.POW_EINVAL and "LIMIT" in msg
    for ctx, t, o in ((None, ctypes.byref(tmpl), ctypes.byref(out)),):
        rc, msg = call(ctx, t, LIMIT - 1, 1, 9, o)  # the last trial is in range
        assert rc == _lib.POW_EINVAL and "null" in msg
    assert bytes(out) == before and found.value == 0x1111 and hashes.value == 0x2222
