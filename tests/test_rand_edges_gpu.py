"""pow_mine_rand (K8) on the GPU at its edges: the proof-of-work compare at
the 32-bit seam (tests/golden/rand_seam.json), windows in which every trial
must be hashed exactly once, the answer at every position of a lane's run and
on both sides of a hop, the shipped plan beyond its first pass, T at its
maximum, templates with layout traps, and the seeds at 32-bit extremes.

Every expected value is tests/rand_util.py's and hashlib's, which never run
the code under test; every comparison of a block is over all 552 bytes.  The
S2 windows share ONE pass of the brute force over trials [0, 2^19 + 1024)
(`s2`: every trial with 15 or more leading zero bits), from which the answer
of any window inside it at any d >= 15 follows."""
import contextlib
import ctypes
import json
import os

import pytest

import rand_util
from mpi_blockchain_amd.block import field, make_block, set_field
from mpi_blockchain_amd.miner import GpuMiner

from helpers import block_from_template
from rand_gpu_util import POISON, SEED, block_of, brute, call, check_against, check_against_brute, miner_with, raw

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCAN = (1 << 19) + 1024

# (POW_RAND_RUN, POW_RAND_LANES_LOG2, POW_RAND_LAUNCH_LOG2) of the test library; None: the shipped library
SHAPES = {"shipped": None, "T4_G256": (4, 8, None), "T64_G512": (64, 9, None), "T1024_G256": (1024, 8, None),
          "T64_G256_launch4096": (64, 8, 12), "T4_G256_launch1024": (4, 8, 10)}


def lz_of(hexd: str) -> int:
    return 256 - int(hexd, 16).bit_length()


@pytest.fixture(scope="module")
def miners():
    """One context per shape, made when first asked for."""
    with contextlib.ExitStack() as stack:
        made = {}

        def get(shape: str):
            if shape not in made:
                if SHAPES[shape] is None:
                    made[shape] = stack.enter_context(GpuMiner(0))
                else:
                    run, lanes, launch = SHAPES[shape]
                    sw = dict(POW_RAND_RUN=run, POW_RAND_LANES_LOG2=lanes)
                    if launch is not None:
                        sw["POW_RAND_LAUNCH_LOG2"] = launch
                    made[shape] = stack.enter_context(miner_with(**sw))
            return made[shape]

        yield get


@pytest.fixture(scope="module")
def s2(templates):
    """Template S2 and every trial of [0, SCAN) with 15 or more leading zero bits, in order."""
    tmpl = block_from_template(templates["S2"])
    hits = brute(raw(tmpl), SEED, 0, SCAN, 15, SCAN)
    # the trials the cases below are laid out around
    assert [h[0] for h in hits[:4]] == [3013, 19644, 55589, 137383]
    assert [(h[0], lz_of(h[2])) for h in hits if lz_of(h[2]) >= 17] == [(180835, 17), (249501, 19)]
    return tmpl, hits


def answer(hits, start: int, count: int, d: int):
    """The lowest solving trial of [start, start + count) at d >= 15, from the shared pass."""
    assert d >= 15 and 0 <= start and start + count <= SCAN
    return next((h for h in hits if start <= h[0] < start + count and lz_of(h[2]) >= d), None)


def layout(m, shape: str, d: int = 15):
    """(T, G, trials per launch) the cases of `shape` are laid out around: the
    forced ones as forced; the shipped plan's for a window of at least 4 x 2^d
    trials (lanes for 4 x 2^d trials, one workgroup per CU and 256 at most, the
    least T whose pass covers them)."""
    if SHAPES[shape] is not None:
        run, lanes, launch = SHAPES[shape]
        return run, 1 << lanes, 1 << (26 if launch is None else launch)
    g = 256 * min(m.device_info()["cu_count"], 256, (4 << d) // 256)
    t = 1
    while t < 1024 and g * t < 4 << d:
        t *= 2
    return t, g, 1 << 26


# ---- a: the 32-bit seam ----
@pytest.fixture(scope="module")
def seam(templates):
    with open(os.path.join(ROOT, "tests", "golden", "rand_seam.json")) as f:
        v = json.load(f)
    rows = v["witnesses"]
    assert sorted(min(r["leading_zeros"], 32) for r in rows) == [31, 32]
    for r in rows:  # every row again, before it is used
        tb = raw(block_from_template(templates[r["template"]]))
        nonce, = rand_util.nonces(r["seed"], r["trial"], 1)
        assert nonce == r["nonce"].encode() + b"\0"
        hit, = rand_util.mine(tb, r["seed"], r["trial"], 1, 0)
        assert hit == (r["trial"], nonce, r["digest"]) and lz_of(r["digest"]) == r["leading_zeros"]
        assert r["trial"] >= v["before"]
    return v


@pytest.mark.parametrize("shape", ["shipped", "T4_G256"])
def test_seam(miners, templates, seam, shape):
    """H0 <= thr where H0 == thr: thr = 1 at d = 31 and thr = 0 at d = 32."""
    m = miners(shape)
    for r in seam["witnesses"]:
        tmpl = block_from_template(templates[r["template"]])
        tb, seed, trial, lz = raw(tmpl), r["seed"], r["trial"], r["leading_zeros"]
        hit = (trial, r["nonce"].encode() + b"\0", r["digest"])
        start = trial - seam["before"]
        for d in (29, 30, 31, 32):
            hits = brute(tb, seed, start, seam["window"], d)
            assert list(hits) == ([hit] if d <= lz else [])  # the witness is alone in its window
            rc, out, found, hashes = call(m, tmpl, seed, start, seam["window"], d)
            if d <= lz:
                assert (rc, found) == (1, trial), (shape, d, lz, m.L.pow_last_error())
                assert out == rand_util.seal(tb, hit[1], hit[2])
                assert seam["before"] + 1 <= hashes <= seam["window"]
            else:
                assert (rc, out, found, hashes) == (0, POISON, 12345, seam["window"]), (shape, d, lz)
        # the witness alone: solves at its own count of zero bits, not at one more
        check_against(m, tmpl, seed, trial, 1, min(lz, 32), hit, every_trial=True)
        if lz + 1 <= 32:
            check_against(m, tmpl, seed, trial, 1, lz + 1, None, every_trial=True)


# ---- b: no trial skipped, none twice ----
GAP = (55590, 137383)  # no trial of [55590, 137383) has 15 zero bits: 81,793 trials


@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_trial_of_an_empty_window_is_hashed_once(miners, s2, shape):
    """A lane counts one per digest, the runs partition the launch and nothing
    stops early without a hit: hashes == count, whatever cuts the last run."""
    tmpl, hits = s2
    m = miners(shape)
    t, g, launch = layout(m, shape)
    d_free = max(lz_of(h[2]) for h in hits) + 1  # no trial of [0, SCAN) has that many zero bits
    assert d_free <= 32
    counts = [1, t - 1, t, t + 1, g * t - 1, g * t, g * t + 1, 2 * g * t + t // 2,
              5 * launch + 333 if launch < 1 << 26 else 12345]  # odd, and no multiple of the launch
    assert all(c >= 1 for c in counts) and counts[-1] % 2 == 1 and counts[-1] % launch
    for count in counts:
        # between two recorded hits at d = 15 where the window fits there; a pass of 2^17 trials and
        # more fits between no two of them: then from trial 0 at the first d that leaves [0, SCAN) empty
        start, d = (GAP[0], 15) if count <= GAP[1] - GAP[0] else (0, d_free)
        assert answer(hits, start, count, d) is None
        got = check_against(m, tmpl, SEED, start, count, d, None, every_trial=True)
        assert got == count
        assert m.stats()["launches"] == -(-count // launch), (shape, count)


# ---- c: the answer at every position of a run, and on both sides of a hop ----
@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_answer_at_every_position_of_a_run(miners, s2, shape):
    tmpl, hits = s2
    m = miners(shape)
    t, g, launch = layout(m, shape)
    # 137383 at d = 15 has 81,793 free trials below it; where 2 G T + T / 2 is more than that, 249501
    # at d = 18 with 249,500 (180835 has 17 zero bits), and the distances that still fit below it
    star, d = (137383, 15) if 2 * g * t + t // 2 <= 81793 else (249501, 18)
    free = star - 1 - max([h[0] for h in hits if h[0] < star and lz_of(h[2]) >= d], default=-1)
    assert (star, d, free) in ((137383, 15, 81793), (249501, 18, 249501))
    dist = [r for r in (0, 1, t - 1, t, t + 1, g * t - t, g * t - 1, g * t, g * t + 1, 2 * g * t + t // 2) if r <= free]
    assert len(dist) >= 5 and (len(dist) == 10 or t * g >= 1 << 17)
    for r in dist:
        start = star - r
        for count in (r + 1, r, r + 1000):  # the answer is the window's last trial; nothing; further trials behind it
            if count == 0:
                continue
            hit = answer(hits, start, count, d)
            assert (hit is None) == (count == r) and (hit is None or hit[0] == star)
            check_against(m, tmpl, SEED, start, count, d, hit, every_trial=True)
            if launch < 1 << 26:  # launches up to the one that holds the answer, or all of them
                assert m.stats()["launches"] == (r // launch + 1 if hit else -(-count // launch)), (shape, r, count)


# ---- d: the shipped plan beyond its first pass ----
@pytest.mark.parametrize("d,start,want", [(9, 370730, 374026), (11, 188578, 197742), (13, 19645, 53248)])
def test_shipped_plan_beyond_its_first_pass(miners, s2, d, start, want):
    """The plan's lanes cover 4 x 2^d trials in one pass; these answers lie behind them."""
    tmpl, _ = s2
    (trial, _, _), = brute(raw(tmpl), SEED, start, 1 << 20, d)
    assert trial == want and trial - start >= 4 << d
    m = miners("shipped")
    assert check_against_brute(m, tmpl, SEED, start, 1 << 20, d) == want
    assert m.stats()["launches"] == 1
    # ... as the window's last trial, and one shorter
    assert check_against_brute(m, tmpl, SEED, start, want - start + 1, d) == want
    assert check_against_brute(m, tmpl, SEED, start, want - start, d) is None


# ---- e: T > 1 in the shipped plan, and T at its maximum ----
def test_long_runs(miners, s2):
    tmpl, hits = s2
    first17 = answer(hits, 0, 1 << 18, 17)
    assert first17[0] == 180835
    m = miners("shipped")
    assert m.device_info()["cu_count"] * 256 < 4 << 17  # one trial per lane does not cover 4 x 2^17: T > 1
    check_against(m, tmpl, SEED, 0, 1 << 18, 17, first17, every_trial=True)
    assert 180835 == 176 * 1024 + 611  # T = 1,024 on 256 lanes: lane 176, draw 611 of its first run
    with miner_with(POW_RAND_RUN=1024, POW_RAND_LANES_LOG2=8) as f:
        check_against(f, tmpl, SEED, 0, 1 << 18, 17, first17, every_trial=True)
        assert f.stats()["launches"] == 1
    assert 256 * 512 <= 180835 < 2 * 256 * 512  # T = 512: the second pass, behind a hop of x^(9 512 255)
    with miner_with(POW_RAND_RUN=512, POW_RAND_LANES_LOG2=8) as f:
        check_against(f, tmpl, SEED, 0, 1 << 18, 17, first17, every_trial=True)
    # one context, T changing from call to call: the tables are made again each time
    for d in (9, 17, 9, 15, 9):
        hit = answer(hits, 0, 1 << 18, d) if d >= 15 else brute(raw(tmpl), SEED, 0, 1 << 18, d)[0]
        check_against(m, tmpl, SEED, 0, 1 << 18, d, hit, every_trial=True)


# ---- f: layout traps ----
def trap_template(index, seed):
    """tests/test_batch_gpu.py's: no NUL anywhere in prev, junk behind block_hash[64], marked padding."""
    import random

    rng = random.Random(seed)
    t = make_block(index, 0x1FF, 3, (1 << 40) + 5 + seed, nonce=b"nnnnnnnnnn",
                   prev=bytes(rng.randrange(1, 256) for _ in range(256)))
    set_field(t, "block_hash", bytes(rng.randrange(1, 256) for _ in range(256)))
    ctypes.memset(ctypes.addressof(t) + 12, 0xEE, 4)   # the padding behind difficulty ...
    ctypes.memset(ctypes.addressof(t) + 546, 0xDD, 6)  # ... and behind block_hash
    return t


def test_layout_traps(miners, templates):
    """K8 builds the message's first word itself from the low bytes of index,
    owner, difficulty and created_at, and the host seals the block."""
    m = miners("shipped")
    s3 = block_from_template(templates["S3"])
    assert (s3.index, s3.node_owner_number, s3.difficulty) == (0xDEADBE80, 0xFFFFFFFF, 0x1FF)
    assert s3.created_at == (1 << 64) - 1 and field(s3, "previous_block_hash") == bytes(range(256))
    traps = [trap_template(0x1FE, 1), trap_template(0xFFFFFFFF, 2), trap_template(7, 3)]
    for tmpl in [s3] + traps:
        tb = raw(tmpl)
        for d in (6, 9):
            assert check_against_brute(m, tmpl, SEED, 0, 1 << 16, d) is not None
            (trial, nonce, hexd), = brute(tb, SEED, 0, 1 << 16, d)
            rc, out, found, _ = call(m, tmpl, SEED, 0, 1 << 16, d)
            assert (rc, found) == (1, trial)
            assert out[:24] == tb[:24] and out[34:290] == tb[34:290]  # header, padding behind difficulty, prev
            assert out[24:33] == nonce[:9] and out[33] == 0           # nonce[9] = 0
            assert out[290:354] == hexd.encode() and out[354] == 0    # the hex text and block_hash[64] = 0
            assert out[355:] == tb[355:]                              # block_hash[65..255] and the padding stay
            # in place: out = tmpl
            t2 = block_of(tb)
            assert m.L.pow_mine_rand(m.ctx, ctypes.byref(t2), SEED, 0, 1 << 16, d, None, 0, ctypes.byref(t2), None,
                                     None) == 1
            assert raw(t2) == out
    for t in traps:
        tb = raw(t)
        assert tb[12:16] == b"\xEE" * 4 and tb[546:] == b"\xDD" * 6 and b"\0" not in tb[34:290] + tb[290:546]


# ---- g: seeds ----
SEEDS = (0, 1, 0x80000000, 0xFFFFFFFF, 1700000003)


@pytest.mark.parametrize("shape", [None, dict(POW_RAND_RUN=16, POW_RAND_LANES_LOG2=9)], ids=["shipped", "T16_G512"])
def test_seeds(miners, templates, shape):
    tmpl = block_from_template(templates["S2"])
    start = 1234577
    with (contextlib.nullcontext(miners("shipped")) if shape is None else miner_with(**shape)) as m:
        for d in (9, 13):
            outs = {}
            for seed in SEEDS:
                assert check_against_brute(m, tmpl, seed, start, 1 << 20, d) is not None
                outs[seed] = call(m, tmpl, seed, start, 1 << 20, d)[:3]
            assert outs[0] == outs[1]  # srand(0) is srand(1)
            assert len({o[1] for o in outs.values()}) == len(SEEDS) - 1
