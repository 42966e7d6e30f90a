"""pow_find_seed on the host (CPU only): its plan, the target packing and the
kernel's index arithmetic in tests/seed_plan_unit.cpp, a process of its own under
sanitizers; the argument checks in their stated order; and the brute force of
tests/seed_util.py, the GPU tests' yardstick, against what the reference's own
gen_random_nonce gave (tests/golden/rand_replay.json)."""
import ctypes
import os
import subprocess

import rand_util
import seed_util
from mpi_blockchain_amd import _lib
from mpi_blockchain_amd.block import nonce_from_counter
from mpi_blockchain_amd.miner import rand_nonces

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 1 << 56


def test_the_name_is_exported():
    assert "pow_find_seed" in _lib.EXPORTS
    assert _lib.load().pow_find_seed and _lib.load(test_hooks=True).pow_find_seed
    assert (_lib.SEED_MAX_SEEDS, _lib.SEED_MAX_TARGETS) == (1 << 20, 64)
    assert ctypes.sizeof(_lib.SeedMatchRec) == 16 and _lib.SeedMatchRec.trial.offset == 8


def test_plan_packing_seeding_and_lane_walk_under_sanitizers(tmp_path):
    """tests/seed_plan_unit.cpp links pow_host.cpp alone and runs as a process
    of its own under ASan + UBSan: nothing is loaded into Python."""
    csrc = os.path.join(ROOT, "mpi_blockchain_amd", "csrc")
    exe = str(tmp_path / "seed_plan_unit")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I", csrc,
                    os.path.join(ROOT, "tests", "seed_plan_unit.cpp"), os.path.join(csrc, "pow_host.cpp"), "-o", exe],
                   check=True, cwd=str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert " checks, 0 failed" in r.stdout, r.stdout
    assert int(r.stdout.split(" checks, 0 failed")[0].split()[-1]) > 1_000_000  # the sweep ran


def test_einval_in_the_stated_order():
    """n_targets, n_seeds, trial_count, the trial range, the null pointers, the
    alphabet: each case has every LATER fault too, and the message names the
    first.  (The seventh, a context bound to a stop board, needs a context:
    tests/test_seed_gpu.py.)  Nothing is written."""
    L = _lib.load()
    good = b"abcXYZ019\0"
    bad = b"abc-YZ019\0"
    out = (_lib.SeedMatchRec * 4)()
    ctypes.memset(out, 0xA5, ctypes.sizeof(out))
    n_found, pairs = ctypes.c_size_t(0x1111), ctypes.c_uint64(0x2222)

    def call(nonces, n_targets, n_seeds, start, count, ctx=None, o=None, cap=4, nf=None):
        rc = L.pow_find_seed(ctx, nonces, n_targets, 5, n_seeds, start, count, None, 0, o, cap, nf, ctypes.byref(pairs))
        return rc, (L.pow_last_error() or b"").decode()

    for n_targets in (0, 65, 1 << 40):
        rc, msg = call(None, n_targets, 0, LIMIT, 0)
        assert rc == _lib.POW_EINVAL and "n_targets" in msg, msg
    for n_seeds in (0, (1 << 20) + 1, 0xFFFFFFFF):
        rc, msg = call(None, 1, n_seeds, LIMIT, 0)
        assert rc == _lib.POW_EINVAL and "n_seeds" in msg, msg
    for count in (0, (1 << 32) + 1):
        rc, msg = call(None, 64, 1 << 20, LIMIT, count)
        assert rc == _lib.POW_EINVAL and "trial_count" in msg, msg
    for start, count in ((LIMIT, 1), (LIMIT - (1 << 32) + 1, 1 << 32), ((1 << 64) - 1, 1)):
        rc, msg = call(None, 1, 1, start, count)
        assert rc == _lib.POW_EINVAL and "LIMIT" in msg, msg
    fake = ctypes.c_void_p(8)  # never dereferenced: a later check fails first
    nf = ctypes.byref(n_found)
    for ctx, nonces, o, cap, f in ((None, bad, out, 4, nf), (fake, None, out, 4, nf), (fake, bad, out, 4, None),
                                   (fake, bad, None, 4, nf)):
        rc, msg = call(nonces, 1, 1, LIMIT - 1, 1, ctx=ctx, o=o, cap=cap, nf=f)  # the last trial is in range
        assert rc == _lib.POW_EINVAL and "null" in msg, msg
    # a target outside the alphabet: any of the nine bytes, of any target; byte 9 is not looked at
    for at in range(9):
        for c in (0, 0x20, ord("-"), ord("_"), 0x7F, 0xE9, ord("/"), ord(":"), ord("@"), ord("["), ord("`"), ord("{")):
            t = bytearray(good)
            t[at] = c
            rc, msg = call(good + bytes(t), 2, 1, 0, 1, ctx=fake, o=None, cap=0, nf=nf)
            assert rc == _lib.POW_EINVAL and "alphabet" in msg and "target 1" in msg, (at, c, msg)
    assert bytes(out) == b"\xA5" * ctypes.sizeof(out) and n_found.value == 0x1111 and pairs.value == 0x2222


def test_packing_round_trips_through_nonce_from_counter():
    """Any counter nonce is a legal target (62^9 of them) and none is refused for
    its alphabet: with a null context the call goes past the sixth check."""
    L = _lib.load()
    n_found = ctypes.c_size_t(7)
    for ctr in (0, 1, 61, 62, 62**9 - 1, 62**5, 123456789012345):
        rc = L.pow_find_seed(None, nonce_from_counter(ctr), 1, 0, 1, 0, 1, None, 0, None, 0, ctypes.byref(n_found), None)
        assert rc == _lib.POW_EINVAL and b"null" in L.pow_last_error()
    assert n_found.value == 7


def test_seeding_through_2_pow_31():
    """pow_rand_nonces against tests/rand_util.py for the 64 seeds around 2^31,
    where the Lehmer step's signed division changes branch, and far down the
    stream of the two whose state is the generator's most degenerate."""
    for seed in range(0x7FFFFFE0, 0x80000020):
        assert rand_nonces(seed, 0, 64) == rand_util.nonces(seed, 0, 64), hex(seed)
    for seed in range(0x7FFFFFFE, 0x80000003):
        zeros = rand_util.seed_words(seed)[1:31].count(0)
        assert zeros == (30 if seed in seed_util.DEGENERATE else 0), hex(seed)
    for seed in seed_util.DEGENERATE:
        assert rand_util.seed_words(seed)[0] == seed
        assert rand_nonces(seed, seed_util.DEEP, 64) == rand_util.nonces(seed, seed_util.DEEP, 64), hex(seed)
        # ... and what the reference's own gen_random_nonce gave after srand(seed)
        assert seed_util.golden_nonces(seed) == rand_nonces(seed, 0, 64) == rand_util.nonces(seed, 0, 64), hex(seed)
        assert len(set(seed_util.golden_nonces(seed))) == 64  # degenerate in its seeding, not in what it draws


def test_the_inputs_of_the_edge_tests():
    """What tests/test_seed_edges_gpu.py asks of its inputs, and its yardstick
    (the brute force over pow_rand_nonces) against the same search over
    tests/rand_util.py on each of them."""
    ru, ref = seed_util.find_seed_ru, seed_util.find_seed_ref
    hits = seed_util.digit_edge_hits()
    assert len(hits) == 12 and all(hits.values()), hits
    for (at, pair), (seed, trial, n) in hits.items():
        assert tuple(seed_util.digits(n)[at:at + 2]) == pair and rand_nonces(seed, trial, 1)[0][:9] == n
    assert hits[0, (61, 61)] == (1700000003, 1007, b"99Z0FmjmU")
    targets = [n for _, _, n in hits.values()]
    want = ru(targets, 1700000003, 3, 0, 4096)
    assert ref(targets, 1700000003, 3, 0, 4096) == want
    assert sorted(want) == sorted((s, k, t) for k, (s, t, _) in enumerate(hits.values()))
    # the near misses: each target but the last differs from N, two of them let a trial of N through both tables
    stream = seed_util.ru_stream(1700000003, 0, 2048)
    n, a, b = stream[1007], stream[5], stream[6]
    targets = seed_util.near_misses(n, a, b)
    d = [seed_util.digits(t) for t in targets]
    assert len(targets) == 12 and d[0][:2] == d[11][:2] and d[0][2:4] != d[11][2:4]
    assert d[1][2:4] == d[11][2:4] and d[1][:2] != d[11][:2]
    assert [[i for i in range(9) if d[2 + k][i] != d[11][i]] for k in range(9)] == [[k] for k in range(9)]
    assert ref(targets, 1700000003, 1, 0, 2048) == ru(targets, 1700000003, 1, 0, 2048) == [(1700000003, 11, 1007)]
    # 64 equal targets under the twin seeds 0 and 1
    targets = [rand_util.nonces(1, 5, 1)[0]] * 64
    want = [(s, k, 5) for s in (0, 1) for k in range(64)]
    assert ref(targets, 0xFFFFFFFE, 4, 0, 64) == ru(targets, 0xFFFFFFFE, 4, 0, 64) == want


def test_brute_force_agrees_with_the_reference_s_recorded_nonces():
    """find_seed_ref, the GPU tests' yardstick, on the golden file: every
    recorded nonce is found at its (seed, trial), with the 0/1 twin where the
    window holds it, and nothing else is."""
    v = seed_util.replay()
    for seed_s, table in v["nonces"].items():
        seed = int(seed_s)
        nonces = seed_util.golden_nonces(seed)
        assert len(nonces) == len(table) == 64
        got = seed_util.find_seed_ref(nonces, seed, 1, 0, 64)
        assert got == [(seed, t, t) for t in range(64)]
    # seeds 0 and 1 share a stream: a window over both holds every nonce twice
    got = seed_util.find_seed_ref(seed_util.golden_nonces(1)[:3], 0xFFFFFFFF, 3, 0, 8)
    assert got == [(s, t, t) for s in (0, 1) for t in range(3)]
    for r in v["replays"]:
        nonces = [bytes.fromhex(b["block_hex"])[24:34] for b in r["blocks"]]
        got = seed_util.find_seed_ref(nonces, r["seed"] - 3, 7, 0, r["total_trials"])
        want = [(s, k, b["trial"]) for s in sorted({r["seed"]} | ({0, 1} if r["seed"] in (0, 1) else set()),
                                                   key=lambda s: (s - (r["seed"] - 3)) & 0xFFFFFFFF)
                for k, b in sorted(enumerate(r["blocks"]), key=lambda kb: kb[1]["trial"])]
        assert got == want, (r["seed"], got, want)
