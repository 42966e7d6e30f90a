"""The 32-bit difficulty seam on the GPU.  Every kernel changes its
proof-of-work test there: K1 and K1' go from H0 <= thr (thr = 0 at d = 32) to
the full-width count above 32, K3 counts over eight words at every d, K4, K5
and K6 (pow_mine_chain, pow_mine_batch, pow_mine_race) compare H0 <= thr up to
32 and leave d > 32 to their host loops over pow_mine.  The witnesses
(tests/golden/lz_witnesses.json) are digests with exactly 31, 32 and 33 leading
zero bits, so each side of the seam has an accept and a reject.

Every expected value is hashlib's (seam_util, the host statements
block.mine_chain, block.mine_batch, block.mine_race and block.verify_chain) or
Python's bit_length."""
import ctypes

import numpy as np
import pytest

from mpi_blockchain_amd._lib import Block, load
from mpi_blockchain_amd.block import V_WORK, field, make_block, mine_batch, mine_chain, mine_race, set_field
from mpi_blockchain_amd.miner import GpuMiner, refresh_template
from oracle.oracle import py_nonce_from_counter

import batch_util as bu
import chain_util as cu
import helpers
import race_util as ru
import seam_util as su
import verify_util as vu

pytestmark = pytest.mark.gpu

SWITCHES = ("POW_FORCE_FULL", "POW_LAT_MAX", "POW_LAT_WPS", "POW_CHAIN_BATCH", "POW_CHAIN_FUSED_MAX",
            "POW_CHAIN_LANES_LOG2", "POW_BATCH_FUSED_MAX", "POW_BATCH_TILE", "POW_BATCH_LANES_LOG2", "POW_RACE_FUSED_MAX",
            "POW_RACE_BATCH", "POW_RACE_LANES_LOG2")
# The shipped library; K1 only (no latency kernel); the d > 32 variants at every
# d; and K1' at 4 waves per SIMD (its asm-group variant) with the d > 32 test:
# pow_mine runs K1' only at d <= 21, so this is its only route to K1'<FULL>.
CONTEXTS = {"shipped": None, "k1_only": {"POW_LAT_MAX": 0}, "force_full": {"POW_FORCE_FULL": 1},
            "lat_asm_full": {"POW_LAT_WPS": 4, "POW_FORCE_FULL": 1}}


def miner_with(**switches):
    """A context of the test library whose pow_init saw exactly these switches."""
    return helpers.hooked_miner(SWITCHES, **switches)


@pytest.fixture(scope="module", params=list(CONTEXTS))
def ctx(request):
    env = CONTEXTS[request.param]
    if env is None:
        with GpuMiner(0) as m:
            yield m
    else:
        with miner_with(**env) as m:
            yield m


def seam_template(templates, name) -> Block:
    """The golden.json template with a block_hash full of bytes that a sealed
    block must keep behind its 65 (node.cpp:318 is a strcpy)."""
    b = helpers.block_from_template(templates[name])
    set_field(b, "block_hash", bytes(1 + (7 * k) % 255 for k in range(256)))
    return b


def sealed(tmpl: Block, t: dict, ctr: int) -> bytes:
    """All 552 bytes of the template sealed with counter ctr, by hashlib."""
    want = helpers.with_nonce(tmpl, py_nonce_from_counter(ctr))
    ctypes.memmove(ctypes.addressof(want) + Block.block_hash.offset, su.digest_of(t, ctr).hex().encode() + b"\0", 65)
    return cu.raw([want])


def check_window(m, tmpl, t, start, count, d, must_solve=None):
    """pow_sweep, pow_sweep_device, pow_mine and pow_mine_any over one window
    against hashlib's list of it."""
    want = su.want_list(t, start, count, d)
    if must_solve is not None:
        assert (len(want) > 0) == must_solve, (start, count, d, want)
    assert m.sweep(tmpl, start, count, d).tolist() == want, (start, count, d)
    assert m.sweep_count(tmpl, start, count, d) == (len(want), start + want[0] if want else None), (start, count, d)
    r = m.mine(tmpl, start, count, d)
    if not want:
        assert r is None and m.mine(tmpl, start, count, d, any_solution=True) is None, (start, count, d)
        return want
    assert r is not None and r.counter == start + want[0], (start, count, d, r and r.counter)
    assert cu.raw([r.block]) == sealed(tmpl, t, r.counter)
    a = m.mine(tmpl, start, count, d, any_solution=True)
    assert a is not None and a.counter - start in want, (start, count, d, a and a.counter)
    assert cu.raw([a.block]) == sealed(tmpl, t, a.counter)
    return want


# ---- B: K1 and K1' ----
@pytest.mark.parametrize("name", list(su.SOLVES))
def test_search_kernels_at_the_seam(ctx, templates, name):
    t, tmpl = templates[name], seam_template(templates, name)
    row = next(r for r in su.seam_rows() if r["template"] == name)
    ctr, lz = row["counter"], row["leading_zeros"]
    start = ctr - su.BEFORE
    for d in su.SEAM_D:
        want = check_window(ctx, tmpl, t, start, su.WINDOW, d, must_solve=d <= lz if d >= 30 else True)
        if d >= 30:
            assert want == ([su.BEFORE] if d <= lz else [])
    # a window the lists above cannot pass empty: about 2,048 / 16 solutions
    assert len(check_window(ctx, tmpl, t, start, su.WINDOW, 4, must_solve=True)) >= 90


@pytest.mark.parametrize("name", list(su.SOLVES))
def test_witness_at_the_window_edges(ctx, templates, name):
    """The witness as a window's first counter, its second, its 62nd (another
    lane of the first chunk's edge mask) and its last; and just past its end."""
    t, tmpl = templates[name], seam_template(templates, name)
    row = next(r for r in su.seam_rows() if r["template"] == name)
    ctr, lz = row["counter"], row["leading_zeros"]
    for d in (lz, lz + 1):
        for start, count in ((ctr, su.WINDOW), (ctr - 1, su.WINDOW), (ctr - 61, su.WINDOW),
                             (ctr - su.BEFORE, su.BEFORE + 1)):
            want = check_window(ctx, tmpl, t, start, count, d, must_solve=d == lz)
            assert want == ([ctr - start] if d == lz else [])
        check_window(ctx, tmpl, t, ctr - su.BEFORE, su.BEFORE, d, must_solve=False)  # ends at ctr, exclusive


# ---- C: K3's work flag at every difficulty ----
@pytest.fixture(scope="module")
def shipped():
    with GpuMiner(0) as m:
        yield m


@pytest.mark.parametrize("name", list(su.SOLVES))
def test_verify_work_flag_at_every_difficulty(shipped, templates, name):
    """child (sealed with hashlib at d = 0), the witness block, a parent whose
    block_hash is the witness's previous_block_hash: POW_V_WORK of the witness
    block is set iff d exceeds its leading zero bits, and every status byte is
    the mirror's, at every d in 0..256."""
    t = templates[name]
    row = next(r for r in su.seam_rows() if r["template"] == name)
    w = helpers.with_nonce(helpers.block_from_template(t), py_nonce_from_counter(row["counter"]))
    set_field(w, "block_hash", row["digest"].encode())
    assert vu.leading_zero_bits(w) == row["leading_zeros"]
    parent = make_block(w.index - 1, 1, 9, 1_700_000_000, block_hash=field(w, "previous_block_hash"))
    child = make_block(w.index + 1, 2, 9, 1_700_000_100, prev=field(w, "block_hash"))
    vu.seal(child, 0, 12345)
    chain = (Block * 3)(child, w, parent)
    lzs = [vu.leading_zero_bits(b) for b in chain]
    base = vu.mirror(chain, 0)
    assert base[0] == 0 and base[1] == 0  # the child and the witness block are valid at d = 0
    for d in range(257):
        want = vu.mirror(chain, d)
        assert want == [s | (V_WORK if d > z else 0) for s, z in zip(base, lzs)]
        r = shipped.verify_chain(chain, d)
        assert r.status.tolist() == want, d
        assert bool(r.status[1] & V_WORK) == (d > row["leading_zeros"]), d
        bad = [i for i, s in enumerate(want) if s]
        assert (r.first_bad, r.n_bad, r.ok) == (bad[0] if bad else 3, len(bad), not bad), d


# ---- D: every word of the kernels' leading-zero count ----
def test_leading_zero_bits_of_every_word():
    values = [v for _, v in su.synthetic_digests()] + su.word_digests()
    n = len(values)
    assert n == 513 + 1010
    want = [256 - v.bit_length() for v in values]
    assert set(range(257)) <= set(want)
    for i in range(8):  # word i decides: every earlier word zero, word i not, for each i
        assert any(32 * i <= z < 32 * (i + 1) for z in want[513:])
    words = np.array([[(v >> (32 * (7 - k))) & 0xFFFFFFFF for k in range(8)] for v in values], dtype=np.uint32)
    out = np.full(n, 0xDEAD, dtype=np.uint32)
    L = load(test_hooks=True)
    fn = L.pow_test_leading_zero_bits
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    fn.restype = ctypes.c_int
    with miner_with() as m:
        rc = fn(m.ctx, words.ctypes.data_as(ctypes.c_void_p), n, out.ctypes.data_as(ctypes.c_void_p))
        assert rc == 0, (rc, L.pow_last_error())
        assert out.tolist() == want
        assert fn(m.ctx, None, 0, None) == 0 and fn(m.ctx, None, 1, None) == -1
    assert not hasattr(load(), "pow_test_leading_zero_bits")  # the shipped library does not export it


# ---- F: K4 at d = 31 and 32, the host loop at 33 ----
def chain_case(d, kind):
    c = su.witnesses()["chain"]
    p = c["parent"]
    parent = make_block(p["index"], p["node_owner_number"], p["difficulty"], p["created_at"])
    w = next(r for r in c["witnesses"] if (r["difficulty"], r["kind"]) == (d, kind))
    return parent, c["owner"], [c["created_at"]], w["counter"] - su.BEFORE, w


def check_chain_window(m, d, kind, fused):
    """pow_mine_chain for one block over a witness's window against the host
    statement (hashlib over the same 2,048 counters), all 552 bytes."""
    parent, owner, created, start, w = chain_case(d, kind)
    want = mine_chain(parent, 1, d, owner, created, start, su.WINDOW)
    rc, mined, hashes, out = cu.call(m.L, m.ctx, parent, 1, d, owner, created, start, su.WINDOW)
    if kind == "solves":
        assert len(want) == 1  # the statement says which counter of the window wins
        assert (rc, mined) == (1, 1), (rc, m.L.pow_last_error())
        assert cu.raw(out) == cu.raw(want)
    else:
        assert want == [], "the witness's window holds a real solution: pick another witness"
        assert (rc, mined) == (0, 0), (rc, mined, m.L.pow_last_error())
        assert cu.raw(out) == b"\xA5" * cu.BLOCK_BYTES  # untouched
    s = m.stats()
    assert s["hashes"] == hashes
    if fused:
        assert s["launches"] == 1 and 1 <= hashes <= su.WINDOW  # one K4 launch; a lane tests a counter at most once
    return cu.raw(out)


@pytest.mark.parametrize("d", [31, 32])
def test_fused_chain_at_the_seam(d):
    got = {}
    with miner_with(POW_CHAIN_FUSED_MAX=32) as m:
        for kind in ("solves", "misses"):
            got[kind] = check_chain_window(m, d, kind, fused=True)
    with miner_with(POW_CHAIN_FUSED_MAX=-1) as h:  # the host loop over pow_mine: the same bytes
        for kind in ("solves", "misses"):
            assert check_chain_window(h, d, kind, fused=False) == got[kind]


@pytest.mark.parametrize("d", [31, 32])
def test_fused_chain_lanes_walk_over_the_witness(d):
    """K4's grid is as many lanes as the window has counters, at most one
    workgroup per CU (at d >= 31 whatever POW_CHAIN_LANES_LOG2 says).  A
    window of two such grids with the witness in its second half is therefore
    reached by a lane's second step; a window shorter than a workgroup runs on
    one workgroup, with the witness as its last counter, alone, and left out."""
    parent, owner, created, _, w = chain_case(d, "solves")
    ctr = w["counter"]
    with miner_with(POW_CHAIN_FUSED_MAX=32, POW_CHAIN_LANES_LOG2=0) as m:
        check_chain_window(m, d, "solves", fused=True)
        grid = 256 * m.device_info()["cu_count"]
        for lo, n, solves in ((ctr - grid - 1000, 2 * grid, True), (ctr - 199, 200, True), (ctr, 1, True),
                              (ctr - 200, 200, False)):
            want = mine_chain(parent, 1, d, owner, created, lo, n)
            assert len(want) == (1 if solves else 0)
            rc, mined, hashes, out = cu.call(m.L, m.ctx, parent, 1, d, owner, created, lo, n)
            assert (rc, mined) == ((1, 1) if solves else (0, 0)), (lo, n, rc, m.L.pow_last_error())
            assert cu.raw(out) == (cu.raw(want) if solves else b"\xA5" * cu.BLOCK_BYTES)
            assert m.stats()["launches"] == 1 and 1 <= hashes <= n


def test_chain_above_32_bits_takes_the_host_loop():
    """d = 33 never runs K4, whose test is H0 <= thr: thr = 0 would accept the
    "misses" witness (32 leading zero bits).  The host loop's K1 <FULL> rejects
    it and accepts the 33-bit one, as the statement does."""
    with miner_with(POW_CHAIN_FUSED_MAX=32) as m:
        check_chain_window(m, 33, "solves", fused=False)
        check_chain_window(m, 33, "misses", fused=False)
    with GpuMiner(0) as m:
        check_chain_window(m, 33, "solves", fused=False)
        check_chain_window(m, 33, "misses", fused=False)


# ---- G: K5 and K6 at d = 31 and 32, their host loops at 33 ----
def check_batch_window(m, d, kind, fused):
    """pow_mine_batch with the refreshed templates of owners 5 and 261 (the
    same message: the witness decides both) over a witness's window against
    the host statement, all 552 bytes of both."""
    parent, owner, created, start, w = chain_case(d, kind)
    assert owner == 5
    tmpls = [refresh_template(parent, o, d, created[0]) for o in (5, 261)]
    stated = mine_batch(tmpls, d, start, su.WINDOW)
    rc, solved, hashes, ctrs, out = bu.call(m.L, m.ctx, tmpls, d, start, su.WINDOW)
    if kind == "solves":
        assert [c for _, c in stated] == [w["counter"]] * 2  # the statement says which counter of the window wins
        assert (rc, solved) == (1, 2), (rc, solved, m.L.pow_last_error())
        assert ctrs == [w["counter"]] * 2
    else:
        assert stated == [(None, None)] * 2, "the witness's window holds a real solution: pick another witness"
        assert (rc, solved) == (0, 0), (rc, solved, m.L.pow_last_error())
        assert ctrs == [bu.NONE] * 2
    assert bytes(out) == bu.expected_bytes(stated)  # the fill where nothing solved
    s = m.stats()
    assert s["hashes"] == hashes
    if fused:
        assert s["launches"] == 1 and 2 <= hashes <= 2 * su.WINDOW  # one K5 launch; a lane tests a counter at most once
    return bytes(out), ctrs


def check_race_window(m, d, kind, owners, fused):
    """pow_mine_race for one height with equal created_at over a witness's
    window against the host statement, which hashes rival 6's window too and so
    says who wins."""
    parent, owner, created, start, w = chain_case(d, kind)
    assert owner == 5
    stated = mine_race(parent, 1, d, owners, created * 2, start, su.WINDOW)
    rc, mined, hashes, winners, ctrs, out = ru.call(m.L, m.ctx, parent, 1, d, owners, created * 2, start, su.WINDOW)
    k = len(stated[0])
    if kind == "solves":
        assert k == 1 and stated[2][0] <= w["counter"]  # owner 5 solves at the witness, unless owner 6 does below it
        if stated[2][0] == w["counter"]:
            assert owners[stated[1][0]] == 5
    elif k == 1:
        assert owners[stated[1][0]] == 6  # owner 5's window is empty: only owner 6 can have solved
    assert (rc, mined) == (k, k), (rc, mined, m.L.pow_last_error())
    want_bytes, want_winners, want_ctrs = ru.expected(stated, 1)
    assert (winners, ctrs) == (want_winners, want_ctrs)
    assert bytes(out) == want_bytes
    s = m.stats()
    assert s["hashes"] == hashes
    if fused:
        assert s["launches"] == 1 and 1 <= hashes <= 2 * su.WINDOW  # one K6 launch
    return bytes(out), winners, ctrs


@pytest.mark.parametrize("d", [31, 32])
def test_fused_batch_at_the_seam(d):
    got = {}
    with miner_with(POW_BATCH_FUSED_MAX=32) as m:
        for kind in ("solves", "misses"):
            got[kind] = check_batch_window(m, d, kind, fused=True)
    with miner_with(POW_BATCH_FUSED_MAX=-1) as h:  # the host loop over pow_mine: the same bytes
        for kind in ("solves", "misses"):
            assert check_batch_window(h, d, kind, fused=False) == got[kind]


@pytest.mark.parametrize("owners", [[5, 6], [6, 5]])
@pytest.mark.parametrize("d", [31, 32])
def test_fused_race_at_the_seam(d, owners):
    got = {}
    with miner_with(POW_RACE_FUSED_MAX=32) as m:
        for kind in ("solves", "misses"):
            got[kind] = check_race_window(m, d, kind, owners, fused=True)
    with miner_with(POW_RACE_FUSED_MAX=-1) as h:  # the host loop over pow_mine: the same bytes
        for kind in ("solves", "misses"):
            assert check_race_window(h, d, kind, owners, fused=False) == got[kind]


def test_batch_above_32_bits_takes_the_host_loop():
    """d = 33 never runs K5, whose test is H0 <= thr: thr = 0 would accept the
    "misses" witness (32 leading zero bits).  The host loop's K1 <FULL> rejects
    it and accepts the 33-bit one, as the statement does."""
    with miner_with(POW_BATCH_FUSED_MAX=32) as m:
        check_batch_window(m, 33, "solves", fused=False)
        check_batch_window(m, 33, "misses", fused=False)
    with GpuMiner(0) as m:
        check_batch_window(m, 33, "solves", fused=False)
        check_batch_window(m, 33, "misses", fused=False)


@pytest.mark.parametrize("owners", [[5, 6], [6, 5]])
def test_race_above_32_bits_takes_the_host_loop(owners):
    """As the batch: K6's H0 <= 0 would accept the 32-bit "misses" witness at d = 33."""
    with miner_with(POW_RACE_FUSED_MAX=32) as m:
        check_race_window(m, 33, "solves", owners, fused=False)
        check_race_window(m, 33, "misses", owners, fused=False)
    with GpuMiner(0) as m:
        check_race_window(m, 33, "solves", owners, fused=False)
        check_race_window(m, 33, "misses", owners, fused=False)
