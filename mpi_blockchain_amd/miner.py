"""GPU miner: the proof_of_work hot path (node.cpp:278-332) on one MI355X.

:class:`GpuMiner` owns one ``pow_ctx`` (one GPU, one HIP stream).  Like the
reference's mining pthread it is driven by exactly one thread; other threads
may only bump the cancel word (:meth:`GpuMiner.cancel`).
"""
from __future__ import annotations

import ctypes
import time
import weakref
from dataclasses import dataclass

import numpy as np

from ._lib import (HASH_SIZE, NONCE_SIZE, POOL_NONE, POW_ENOSPC, POW_KEEP_BY_INDEX, POW_KEEP_SOUND_ONLY,
                   POW_TIPS_SOUND_ONLY, SEED_MAX_SEEDS, SEED_MAX_TARGETS, Block, PoolInfo, PoolLiftInfo, PowStats,
                   SeedMatchRec, check, load)
from .block import DEFAULT_DIFFICULTY, field, nonce_from_counter


@dataclass
class MineResult:
    block: Block          # the solved block (nonce + block_hash filled)
    counter: int          # counter whose nonce solved it (lowest in range)
    hashes: int           # trials issued
    kernel_ms: float      # GPU time of the call


@dataclass
class VerifyResult:
    ok: bool              # every block passed (pow_verify_chain returned 1)
    first_bad: int        # lowest flagged index; len(chain) if none
    n_bad: int            # flagged blocks
    status: np.ndarray    # np.uint8 per block: OR of block.V_HASH / V_WORK / V_LINK / V_INDEX


@dataclass
class VerifyChainsResult:
    ok: bool              # no block of any chain is flagged (pow_verify_chains returned 1)
    best: int | None      # the fork choice: the valid chain with the highest tip index (lowest position on a tie); None if none
    first_bad: list       # per chain: the lowest flagged index within it; its length if none
    n_bad: list           # per chain: flagged blocks
    status: list          # per chain: np.uint8 per block, as VerifyResult.status


@dataclass
class IndexBlocksResult:
    ok: bool              # no block of the pool is flagged (pow_index_blocks returned 1)
    best: int | None      # the fork choice: the block with n_bad == 0 and the highest index (lowest position on a tie); None if none
    status: np.ndarray    # np.uint8 per block, as VerifyResult.status
    parent: np.ndarray    # np.uint32 per block: a pool position, block.POOL_ROOT or block.POOL_NONE
    depth: np.ndarray     # np.uint32 per block: the blocks of the chain under it, itself included
    n_bad: np.ndarray     # np.uint32 per block: the flagged ones among them; 0 = the chain under it is sound


@dataclass
class MineChainResult:
    blocks: ctypes.Array  # the mined chain, tip first: Block * n_mined
    n_mined: int          # blocks mined
    complete: bool        # all n were mined (pow_mine_chain returned 1)
    hashes: int           # trials issued
    kernel_ms: float      # GPU time of the call


@dataclass
class MineBatchResult:
    blocks: list          # per template: the sealed Block, or None where unsolved or unreached
    counters: list        # per template: the lowest solving counter, or None
    n_solved: int         # templates solved
    complete: bool        # all were solved (pow_mine_batch returned 1)
    hashes: int           # trials issued
    kernel_ms: float      # GPU time of the call


@dataclass
class MineRaceResult:
    blocks: ctypes.Array  # the winners' chain, tip first: Block * n_mined
    winners: list         # per mined height, tip first: the winner's position in `owners`
    counters: list        # per mined height, tip first: the winner's counter
    n_mined: int          # heights mined
    complete: bool        # all n were mined (pow_mine_race returned 1)
    hashes: int           # trials issued
    kernel_ms: float      # GPU time of the call


@dataclass
class MineRandResult:
    block: Block          # the solved block (the reference's nonce of `trial` + block_hash filled)
    trial: int            # the lowest solving trial of the window: the reference's stream then stands at trial + 1
    hashes: int           # trials issued
    kernel_ms: float      # GPU time of the call


@dataclass(frozen=True)
class SeedMatch:
    seed: int             # the srand() argument
    trial: int            # absolute trial: rand_nonces(seed, trial, 1) gives the target
    target: int           # index into the nonces that were searched for


@dataclass
class RandProvenance:
    """What :func:`audit_rand_provenance` found; per-owner entries are keyed by
    ``node_owner_number``, per-block ones follow the chain's order."""

    seeds: dict               # owner -> the seed that explains most of its blocks (lowest in the window on a tie); None if none does
    trials: list              # per block: its trial under its owner's seed, or None
    not_from_generator: list  # positions of the blocks no (seed, trial) of the window explains
    one_seed: dict            # owner -> every block of the owner matches under its seed
    seed_in_window: dict      # owner -> that seed minus the owner's rank lies within the seed window
    trials_increase: dict     # owner -> its trials strictly increase with its blocks' index
    matches: list             # every SeedMatch of the search

    @property
    def ok(self) -> bool:
        return bool(self.seeds) and all(all(v.values()) for v in (self.one_seed, self.seed_in_window, self.trials_increase))


def rand_nonces(seed: int, start: int = 0, n: int = 1) -> list[bytes]:
    """pow_rand_nonces: what the reference's gen_random_nonce (block.cpp:61-72)
    returns at calls start .. start + n - 1 after srand(seed), each 9
    characters + NUL.  Host only; no GPU work and no call of rand()."""
    buf = ctypes.create_string_buffer(max(n, 1) * NONCE_SIZE)
    L = load()
    check(L.pow_rand_nonces(seed & 0xFFFFFFFF, start, n, buf), L)
    return [buf.raw[i * NONCE_SIZE:(i + 1) * NONCE_SIZE] for i in range(n)]


def refresh_template(last: Block, rank: int, difficulty: int = DEFAULT_DIFFICULTY,
                     now: int | None = None) -> Block:
    """node.cpp:292-299: copy the last block, index+1, owner = rank,
    difficulty = DEFAULT_DIFFICULTY, created_at = time(NULL), and
    memcpy(prev, last.block_hash, 256) — all 256 bytes (trap T5)."""
    b = Block()
    ctypes.pointer(b)[0] = last
    b.index = (last.index + 1) & 0xFFFFFFFF
    b.node_owner_number = rank & 0xFFFFFFFF
    b.difficulty = difficulty & 0xFFFFFFFF
    b.created_at = int(time.time()) if now is None else now
    ctypes.memmove(ctypes.addressof(b) + Block.previous_block_hash.offset,
                   ctypes.addressof(last) + Block.block_hash.offset, HASH_SIZE)
    return b


class GpuPool:
    """A ``pow_pool`` of a :class:`GpuMiner` (:meth:`GpuMiner.open_pool`): the
    block tree of everything added so far, kept on the GPU.  A context manager;
    driven by the miner's thread."""

    def __init__(self, miner: "GpuMiner", difficulty: int, reserve: int = 0):
        self.miner, self.L = miner, miner.L
        self.handle = ctypes.c_void_p()
        check(self.L.pow_pool_open(miner.ctx, difficulty, reserve, ctypes.byref(self.handle)), self.L)
        miner._pools.add(self)  # the miner closes what is still open before its context goes

    def close(self) -> None:
        if self.handle:
            self.L.pow_pool_close(self.handle)
            self.handle = ctypes.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __len__(self) -> int:
        return self.info()["size"]

    @staticmethod
    def _info(raw: PoolInfo) -> dict:
        d = {name: getattr(raw, name) for name, _ in PoolInfo._fields_}
        d["best"] = None if raw.best == POOL_NONE else raw.best
        return d

    def add(self, blocks) -> dict:
        """pow_pool_add: a list of Blocks or a ctypes ``Block * m`` array.
        Returns the pool's info after the add, with ``ok``: no block of the
        whole pool is flagged."""
        m = len(blocks)
        arr = blocks if isinstance(blocks, ctypes.Array) else (Block * max(m, 1))(*blocks)
        raw = PoolInfo()
        rc = check(self.L.pow_pool_add(self.handle, arr, m, ctypes.byref(raw)), self.L)
        return {**self._info(raw), "ok": rc == 1}

    def info(self) -> dict:
        raw = PoolInfo()
        check(self.L.pow_pool_get_info(self.handle, ctypes.byref(raw)), self.L)
        return self._info(raw)

    def read(self, first: int = 0, count: int | None = None) -> IndexBlocksResult:
        """pow_pool_read: the four per-block results of `count` blocks from
        `first` (all of them by default), with the pool's ``best`` and ``ok``."""
        info = self.info()
        n = info["size"] - first if count is None else count
        status = np.zeros(max(n, 0), dtype=np.uint8)
        parent, depth, bad = (np.zeros(max(n, 0), dtype=np.uint32) for _ in range(3))
        u32p = ctypes.POINTER(ctypes.c_uint32)
        check(self.L.pow_pool_read(self.handle, first, n, status.ctypes.data_as(ctypes.c_void_p),
                                   parent.ctypes.data_as(u32p), depth.ctypes.data_as(u32p),
                                   bad.ctypes.data_as(u32p)), self.L)
        return IndexBlocksResult(info["n_flagged"] == 0, info["best"], status, parent, depth, bad)

    def find(self, names) -> list[int]:
        """pow_pool_find: per name (64 bytes each) the named block's position
        or ``block.POOL_NONE``."""
        names = [bytes(x) for x in names]
        if any(len(x) != 64 for x in names):
            raise ValueError("a name is 64 characters")
        k = len(names)
        pos = (ctypes.c_uint32 * max(k, 1))()
        check(self.L.pow_pool_find(self.handle, b"".join(names), k, pos), self.L)
        return list(pos)[:k]

    @staticmethod
    def _seeds(tips, min_index, sound_only):
        """(tips as a ctypes array, their count, min_index, flags) of pow_pool_mark and pow_pool_prune."""
        tips = [int(t) for t in tips]
        arr = (ctypes.c_uint32 * max(len(tips), 1))(*tips)
        flags = 0 if min_index is None else POW_KEEP_BY_INDEX | (POW_KEEP_SOUND_ONLY if sound_only else 0)
        return arr, len(tips), 0 if min_index is None else min_index, flags

    def mark(self, tips=(), min_index: int | None = None, sound_only: bool = False) -> np.ndarray:
        """pow_pool_mark: per block 1 if it is a seed or lies on the walk from
        one along ``parent``, as a ``numpy.uint8`` array.  The seeds: every
        position in `tips`, and with `min_index` every block of that index or
        more (`sound_only`: only those with ``n_bad == 0``); ``None`` means no
        index seeds.  The host statement is :meth:`block.BlockPool.mark`."""
        arr, k, lo, flags = self._seeds(tips, min_index, sound_only)
        on = np.zeros(len(self), dtype=np.uint8)
        n_on = ctypes.c_size_t()
        check(self.L.pow_pool_mark(self.handle, arr, k, lo, flags, on.ctypes.data_as(ctypes.c_void_p),
                                   ctypes.byref(n_on)), self.L)
        assert n_on.value == int(on.sum())
        return on

    def prune(self, tips=(), min_index: int | None = None, sound_only: bool = False):
        """pow_pool_prune: the pool keeps exactly what :meth:`mark` marks, in
        its order.  Returns ``(map, info)``: per block of the pool before the
        call its new position or ``block.POOL_NONE`` (``numpy.uint32``), and
        the pool's info with ``ok`` as :meth:`add` gives it."""
        arr, k, lo, flags = self._seeds(tips, min_index, sound_only)
        new = np.zeros(len(self), dtype=np.uint32)
        raw = PoolInfo()
        rc = check(self.L.pow_pool_prune(self.handle, arr, k, lo, flags,
                                         new.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), ctypes.byref(raw)), self.L)
        return new, {**self._info(raw), "ok": rc == 1}

    @staticmethod
    def _u32(values) -> np.ndarray:
        return np.ascontiguousarray(np.asarray(values, dtype=np.uint64).astype(np.uint32).reshape(-1))

    def ancestors(self, pos, steps) -> np.ndarray:
        """pow_pool_ancestors: per query the block ``steps[q]`` steps along
        ``parent`` from ``pos[q]``, or the walk's end (``block.POOL_ROOT``,
        ``block.POOL_NONE``), as ``numpy.uint32``.  The host statement is
        :meth:`block.BlockPool.ancestor`."""
        pos, steps = self._u32(pos), self._u32(steps)
        if len(pos) != len(steps):
            raise ValueError("one step count per position")
        u32p = ctypes.POINTER(ctypes.c_uint32)
        out = np.zeros(len(pos), dtype=np.uint32)
        check(self.L.pow_pool_ancestors(self.handle, pos.ctypes.data_as(u32p), steps.ctypes.data_as(u32p), len(pos),
                                        out.ctypes.data_as(u32p)), self.L)
        return out

    def fork_points(self, a, b):
        """pow_pool_fork_points: ``(at, back_a, back_b)`` as ``numpy.uint32``
        arrays; ``at[q]`` is the first block on the walk from ``a[q]`` that
        also lies on the walk from ``b[q]``, or ``block.POOL_NONE``.  The host
        statement is :meth:`block.BlockPool.fork_point`."""
        a, b = self._u32(a), self._u32(b)
        if len(a) != len(b):
            raise ValueError("the queries are pairs")
        u32p = ctypes.POINTER(ctypes.c_uint32)
        at, back_a, back_b = (np.zeros(len(a), dtype=np.uint32) for _ in range(3))
        check(self.L.pow_pool_fork_points(self.handle, a.ctypes.data_as(u32p), b.ctypes.data_as(u32p), len(a),
                                          at.ctypes.data_as(u32p), back_a.ctypes.data_as(u32p),
                                          back_b.ctypes.data_as(u32p)), self.L)
        return at, back_a, back_b

    def chain(self, tip: int, max_len: int | None = None) -> np.ndarray:
        """pow_pool_chain: `tip`, its parent and so on in order, at most
        `max_len` positions (the whole walk by default), as ``numpy.uint32``.
        The host statement is :meth:`block.BlockPool.chain`."""
        room = len(self) if max_len is None else int(max_len)
        out = np.zeros(min(room, len(self)), dtype=np.uint32)
        n = ctypes.c_size_t()
        check(self.L.pow_pool_chain(self.handle, int(tip), room, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                    ctypes.byref(n)), self.L)
        return out[:n.value]

    def tips(self, sound_only: bool = False, cap: int | None = None) -> np.ndarray:
        """pow_pool_tips: the positions nobody names as a parent, ascending, as
        ``numpy.uint32`` (`sound_only`: only those with ``n_bad == 0``).  With
        `cap` at most that many; ``self.n_tips`` holds the total of the last
        call either way.  The host statement is :meth:`block.BlockPool.tips`."""
        room = len(self) if cap is None else int(cap)
        out = np.zeros(max(room, 1), dtype=np.uint32)
        n = ctypes.c_size_t()
        rc = self.L.pow_pool_tips(self.handle, POW_TIPS_SOUND_ONLY if sound_only else 0,
                                  out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), room, ctypes.byref(n))
        if rc != POW_ENOSPC:
            check(rc, self.L)
        self.n_tips = n.value
        return out[:min(room, n.value)]

    def subtrees(self, roots, marks: bool = False):
        """pow_pool_subtrees: ``(size, height, best, best_index)`` per root as
        ``numpy.uint32`` arrays (``best`` is ``block.POOL_NONE`` where no member
        has ``n_bad == 0``); with `marks` a fifth result, per block 1 if it is a
        member of any root's subtree (``numpy.uint8``).  The host statement is
        :meth:`block.BlockPool.subtrees`."""
        roots = self._u32(roots)
        k = len(roots)
        u32p = ctypes.POINTER(ctypes.c_uint32)
        size, height, best, best_index = (np.zeros(k, dtype=np.uint32) for _ in range(4))
        on = np.zeros(len(self), dtype=np.uint8) if marks else None
        n_on = ctypes.c_size_t()
        check(self.L.pow_pool_subtrees(self.handle, roots.ctypes.data_as(u32p), k, size.ctypes.data_as(u32p),
                                       height.ctypes.data_as(u32p), best.ctypes.data_as(u32p),
                                       best_index.ctypes.data_as(u32p),
                                       on.ctypes.data_as(ctypes.c_void_p) if marks else None,
                                       ctypes.byref(n_on) if marks else None), self.L)
        if not marks:
            return size, height, best, best_index
        assert n_on.value == int(on.sum())
        return size, height, best, best_index, on

    def drop(self, roots):
        """pow_pool_drop: the pool loses every block of every root's subtree
        and keeps the rest in its order.  Returns ``(map, info)`` as
        :meth:`prune` does.  The host statement is :meth:`block.BlockPool.drop`."""
        roots = self._u32(roots)
        new = np.zeros(len(self), dtype=np.uint32)
        raw = PoolInfo()
        u32p = ctypes.POINTER(ctypes.c_uint32)
        rc = check(self.L.pow_pool_drop(self.handle, roots.ctypes.data_as(u32p), len(roots), new.ctypes.data_as(u32p),
                                        ctypes.byref(raw)), self.L)
        return new, {**self._info(raw), "ok": rc == 1}

    def lift_info(self) -> dict:
        """pow_pool_lift_get_info: the queries' table as the next query will find it."""
        raw = PoolLiftInfo()
        check(self.L.pow_pool_lift_get_info(self.handle, ctypes.byref(raw)), self.L)
        return {name: getattr(raw, name) for name, _ in PoolLiftInfo._fields_}


class GpuMiner:
    def __init__(self, device: int = 0, test_hooks: bool = False):
        """test_hooks=True: a context of libpow_gpu_test.so, which reads the
        test switches (POW_FORCE_FULL, POW_LAT_MAX, POW_GRID_PER_CU, ...) from
        the environment at pow_init; tests only."""
        self.L = load(test_hooks)
        self.ctx = ctypes.c_void_p()
        check(self.L.pow_init(device, ctypes.byref(self.ctx)), self.L)
        self.device = device
        self._cancel = ctypes.c_uint32(0)
        self._pools = weakref.WeakSet()  # open GpuPools: pow_destroy keeps a context that has any

    def warmup(self) -> None:
        """Load every kernel now (HIP loads code objects at first launch)."""
        check(self.L.pow_warmup(self.ctx), self.L)

    # ---- lifecycle ----
    def close(self) -> None:
        if self.ctx:
            for pool in list(self._pools):
                pool.close()
            self.L.pow_destroy(self.ctx)
            self.ctx = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # ---- info ----
    def device_info(self) -> dict:
        cu, clk = ctypes.c_int(), ctypes.c_int()
        name = ctypes.create_string_buffer(256)
        check(self.L.pow_device_info(self.ctx, ctypes.byref(cu), ctypes.byref(clk), name, 256), self.L)
        return {"cu_count": cu.value, "clock_khz": clk.value, "name": name.value.decode()}

    def pci_bus_id(self) -> str:
        """The GPU as "domain:bus:device.function" (pow_device_pci_bus_id)."""
        buf = ctypes.create_string_buffer(64)
        check(self.L.pow_device_pci_bus_id(self.ctx, buf, len(buf)), self.L)
        return buf.value.decode()

    def launch_path(self) -> str:
        """How the latency-bound launches go out (pow_launch_path): "hip"
        (hipLaunchKernel; the shipped library's only path) or "direct" (AQL
        packets into the process's dispatch queue: test library with
        POW_AQL=1)."""
        return "direct" if check(self.L.pow_launch_path(self.ctx), self.L) == 1 else "hip"

    def stats(self) -> dict:
        s = PowStats()
        check(self.L.pow_get_stats(self.ctx, ctypes.byref(s)), self.L)
        return {"kernel_ms": s.kernel_ms, "launches": s.launches, "hashes": s.hashes}

    # ---- block_to_hash (block.cpp:74-77) ----
    def hash_blocks(self, blocks) -> list[str]:
        n = len(blocks)
        if n == 0:
            return []
        arr = (Block * n)(*blocks)
        hx = ctypes.create_string_buffer(65 * n)
        check(self.L.pow_hash_blocks(self.ctx, arr, n, None, hx), self.L)
        raw = hx.raw
        return [raw[65 * i: 65 * i + 64].decode() for i in range(n)]

    def block_to_hash(self, b: Block) -> str:
        return self.hash_blocks([b])[0]

    def digest(self, b: Block) -> bytes:
        dg = ctypes.create_string_buffer(32)
        check(self.L.pow_hash_block(self.ctx, ctypes.byref(b), dg, None), self.L)
        return dg.raw

    # ---- the block tree of a pool (node_blocks walked by previous_block_hash) ----
    def index_blocks(self, pool, difficulty: int = DEFAULT_DIFFICULTY) -> IndexBlocksResult:
        """pow_index_blocks over a pool of blocks in any order: a list of
        Blocks or a ctypes ``Block * n`` array (passed as it is).  The host
        statement of the result is :func:`mpi_blockchain_amd.block.index_blocks`;
        :func:`mpi_blockchain_amd.block.chain_from` extracts a tip's chain."""
        n = len(pool)
        arr = pool if isinstance(pool, ctypes.Array) else (Block * max(n, 1))(*pool)
        status = np.zeros(n, dtype=np.uint8)
        parent, depth, bad = (np.zeros(n, dtype=np.uint32) for _ in range(3))
        u32p = ctypes.POINTER(ctypes.c_uint32)
        best = ctypes.c_size_t()
        rc = check(self.L.pow_index_blocks(self.ctx, arr, n, difficulty, status.ctypes.data_as(ctypes.c_void_p),
                                           parent.ctypes.data_as(u32p), depth.ctypes.data_as(u32p),
                                           bad.ctypes.data_as(u32p), ctypes.byref(best)), self.L)
        return IndexBlocksResult(rc == 1, None if best.value == ctypes.c_size_t(-1).value else best.value,
                                 status, parent, depth, bad)

    def open_pool(self, difficulty: int = DEFAULT_DIFFICULTY, reserve: int = 0) -> "GpuPool":
        """pow_pool_open: an empty pool that stays on the GPU and is fed in
        batches (:class:`GpuPool`; close it before the miner).  The host
        statement is :class:`mpi_blockchain_amd.block.BlockPool`."""
        return GpuPool(self, difficulty, reserve)

    # ---- chain audit (check_first + check_chain + solves_problem for every block) ----
    def verify_chain(self, blocks, difficulty: int = DEFAULT_DIFFICULTY) -> VerifyResult:
        """pow_verify_chain over a chain, tip first: a list of Blocks or a
        ctypes ``Block * n`` array (passed as it is).  The host statement of
        the result is :func:`mpi_blockchain_amd.block.verify_chain`."""
        n = len(blocks)
        arr = blocks if isinstance(blocks, ctypes.Array) else (Block * n)(*blocks)
        status = np.zeros(n, dtype=np.uint8)
        first, bad = ctypes.c_size_t(), ctypes.c_size_t()
        rc = check(self.L.pow_verify_chain(self.ctx, arr, n, difficulty, status.ctypes.data_as(ctypes.c_void_p),
                                           ctypes.byref(first), ctypes.byref(bad)), self.L)
        return VerifyResult(rc == 1, first.value, bad.value, status)

    def verify_chains(self, chains, difficulty: int = DEFAULT_DIFFICULTY) -> VerifyChainsResult:
        """pow_verify_chains over a sequence of chains, each tip first and a
        list of Blocks or a ctypes ``Block`` array (empty chains allowed):
        every chain audited on its own in one call, and the fork choice among
        the valid ones.  The host statements of the result are
        :func:`mpi_blockchain_amd.block.verify_chains` and
        :func:`mpi_blockchain_amd.block.best_chain`."""
        n = len(chains)
        lens = [len(c) for c in chains]
        total = sum(lens)
        arr = (Block * max(total, 1))()
        at = 0
        for c, ln in zip(chains, lens):
            if ln == 0:
                continue
            if isinstance(c, ctypes.Array):
                ctypes.memmove(ctypes.byref(arr, at * ctypes.sizeof(Block)), c, ln * ctypes.sizeof(Block))
            else:
                for i, b in enumerate(c):
                    ctypes.memmove(ctypes.byref(arr, (at + i) * ctypes.sizeof(Block)), ctypes.addressof(b),
                                   ctypes.sizeof(Block))
            at += ln
        lengths = (ctypes.c_uint32 * max(n, 1))(*lens)
        status = np.zeros(total, dtype=np.uint8)
        first = (ctypes.c_uint32 * max(n, 1))()
        bad = (ctypes.c_uint32 * max(n, 1))()
        best = ctypes.c_size_t()
        rc = check(self.L.pow_verify_chains(self.ctx, arr, lengths, n, difficulty,
                                            status.ctypes.data_as(ctypes.c_void_p), first, bad, ctypes.byref(best)),
                   self.L)
        ends = np.cumsum([0] + lens)
        return VerifyChainsResult(rc == 1, None if best.value == ctypes.c_size_t(-1).value else best.value,
                                  list(first)[:n], list(bad)[:n],
                                  [status[ends[c]:ends[c + 1]] for c in range(n)])

    # ---- mining ----
    def cancel(self) -> None:
        """Called from another thread (the receive loop) when the chain moved:
        bumps the cancel word and publishes it to the GPU (pow_cancel), so a
        running mine call stops within one inner step, not at its next
        sub-round."""
        self._cancel.value = (self._cancel.value + 1) & 0xFFFFFFFF
        check(self.L.pow_cancel(self.ctx, self._cancel.value), self.L)

    @property
    def epoch(self) -> int:
        return self._cancel.value

    def bind_board(self, board: "StopBoard | None", slot: int = 0, tag: int = 1) -> None:
        """Join a search shared with other GPUs / contexts (pow_board_bind):
        this miner's hits go to `slot` of `board`, and its mine calls stop as
        soon as a peer slot of the same `tag` makes its remaining counters
        moot.  board=None unbinds."""
        check(self.L.pow_board_bind(self.ctx, board.ptr if board is not None else None, slot, tag), self.L)

    def mine(self, tmpl: Block, start: int = 0, count: int = 1 << 40, difficulty: int = DEFAULT_DIFFICULTY,
             epoch: int | None = None, any_solution: bool = False) -> MineResult | None:
        """Lowest solving counter in [start, start+count) (pow_mine), or the
        first one found (pow_mine_any, lowest latency); None if none / cancelled."""
        out = Block()
        ctr, hashes = ctypes.c_uint64(), ctypes.c_uint64()
        ep = self._cancel.value if epoch is None else epoch
        fn = self.L.pow_mine_any if any_solution else self.L.pow_mine
        rc = check(fn(self.ctx, ctypes.byref(tmpl), start, count, difficulty,
                      ctypes.byref(self._cancel), ep, ctypes.byref(out),
                      ctypes.byref(ctr), ctypes.byref(hashes)), self.L)
        if rc == 0:
            return None
        return MineResult(out, ctr.value, hashes.value, self.stats()["kernel_ms"])

    def mine_rand(self, tmpl: Block, seed: int, start: int = 0, count: int = 1 << 32,
                  difficulty: int = DEFAULT_DIFFICULTY, epoch: int | None = None) -> MineRandResult | None:
        """pow_mine_rand: :meth:`mine` with the reference's own nonces, trials
        [start, start + count) of the stream of ``srand(seed)``: the LOWEST
        solving trial, which is where the reference itself stops.  None if the
        window holds none or :meth:`cancel` was called meanwhile."""
        out = Block()
        trial, hashes = ctypes.c_uint64(), ctypes.c_uint64()
        ep = self._cancel.value if epoch is None else epoch
        rc = check(self.L.pow_mine_rand(self.ctx, ctypes.byref(tmpl), seed & 0xFFFFFFFF, start, count, difficulty,
                                        ctypes.byref(self._cancel), ep, ctypes.byref(out), ctypes.byref(trial),
                                        ctypes.byref(hashes)), self.L)
        if rc == 0:
            return None
        return MineRandResult(out, trial.value, hashes.value, self.stats()["kernel_ms"])

    def find_seed(self, nonces, seed_first: int, n_seeds: int, start: int = 0, count: int = 1 << 32,
                  cap: int = 1024, epoch: int | None = None) -> list[SeedMatch]:
        """pow_find_seed, the inverse of :func:`rand_nonces`: every (seed,
        trial) with seed in [seed_first, seed_first + n_seeds) mod 2^32 and
        trial in [start, start + count) whose nine characters equal one of
        `nonces` (1 to 64 byte strings of at least nine characters), sorted by
        (position of the seed in the window, trial, target).  Seeds 0 and 1
        share a stream and are both reported.  More matches than `cap` raise
        PowError (POW_ENOSPC); [] also if :meth:`cancel` was called meanwhile."""
        nonces = [bytes(n) for n in nonces]
        if any(len(n) < NONCE_SIZE - 1 for n in nonces):
            raise ValueError("a nonce has nine characters")
        buf = b"".join(n[:NONCE_SIZE - 1] + b"\0" for n in nonces)
        out = (SeedMatchRec * max(cap, 1))()
        n_found = ctypes.c_size_t()
        ep = self._cancel.value if epoch is None else epoch
        check(self.L.pow_find_seed(self.ctx, buf, len(nonces), seed_first & 0xFFFFFFFF, n_seeds, start, count,
                                   ctypes.byref(self._cancel), ep, out, cap, ctypes.byref(n_found), None), self.L)
        return [SeedMatch(out[i].seed, out[i].trial, out[i].target) for i in range(n_found.value)]

    def mine_chain(self, parent: Block, n: int, difficulty: int = DEFAULT_DIFFICULTY, owner: int = 0,
                   created_at=None, ctr_start: int = 0, ctr_count: int = 1 << 32,
                   epoch: int | None = None) -> MineChainResult:
        """pow_mine_chain: `n` blocks on top of `parent`, each the child of the
        one before, every one the lowest solving counter of the same window.
        ``blocks`` is the mined chain tip first, a ctypes ``Block * n_mined``
        array (what :meth:`verify_chain` takes); it is shorter than `n` if a
        window held no solution or :meth:`cancel` was called meanwhile.  The
        host statement of the result is :func:`mpi_blockchain_amd.block.mine_chain`."""
        out = (Block * max(n, 1))()
        times = None
        if created_at is not None:
            if len(created_at) != n:
                raise ValueError(f"created_at has {len(created_at)} entries for {n} blocks")
            times = (ctypes.c_uint64 * max(n, 1))(*created_at)
        mined, hashes = ctypes.c_size_t(), ctypes.c_uint64()
        ep = self._cancel.value if epoch is None else epoch
        rc = check(self.L.pow_mine_chain(self.ctx, ctypes.byref(parent), n, difficulty, owner, times, ctr_start,
                                         ctr_count, ctypes.byref(self._cancel), ep, out, ctypes.byref(mined),
                                         ctypes.byref(hashes)), self.L)
        m = mined.value
        blocks = (Block * m)()
        if m:
            ctypes.memmove(blocks, ctypes.byref(out, (n - m) * ctypes.sizeof(Block)), m * ctypes.sizeof(Block))
        return MineChainResult(blocks, m, rc == 1, hashes.value, self.stats()["kernel_ms"])

    def mine_batch(self, tmpls, difficulty: int = DEFAULT_DIFFICULTY, ctr_start: int = 0, ctr_count: int = 1 << 32,
                   epoch: int | None = None) -> MineBatchResult:
        """pow_mine_batch: every template of `tmpls` (a sequence of Blocks or a
        ctypes ``Block`` array) mined on its own over the same window, each the
        lowest solving counter, in one call.  ``blocks[i]`` is the sealed block
        of template i, or None where its window held no solution or
        :meth:`cancel` was called before it was reached.  The host statement of
        the result is :func:`mpi_blockchain_amd.block.mine_batch`."""
        n = len(tmpls)
        arr = (Block * max(n, 1))()
        for i, t in enumerate(tmpls):
            ctypes.memmove(ctypes.byref(arr, i * ctypes.sizeof(Block)), ctypes.addressof(t), ctypes.sizeof(Block))
        out = (Block * max(n, 1))()
        ctrs = (ctypes.c_uint64 * max(n, 1))()
        solved, hashes = ctypes.c_size_t(), ctypes.c_uint64()
        ep = self._cancel.value if epoch is None else epoch
        rc = check(self.L.pow_mine_batch(self.ctx, arr, n, difficulty, ctr_start, ctr_count, ctypes.byref(self._cancel),
                                         ep, out, ctrs, ctypes.byref(solved), ctypes.byref(hashes)), self.L)
        blocks, counters = [], []
        for i in range(n):
            hit = ctrs[i] != 0xFFFFFFFFFFFFFFFF
            b = None
            if hit:
                b = Block()
                ctypes.memmove(ctypes.addressof(b), ctypes.byref(out, i * ctypes.sizeof(Block)), ctypes.sizeof(Block))
            blocks.append(b)
            counters.append(ctrs[i] if hit else None)
        return MineBatchResult(blocks, counters, solved.value, rc == 1, hashes.value, self.stats()["kernel_ms"])

    def mine_race(self, parent: Block, n: int, difficulty: int = DEFAULT_DIFFICULTY, owners=(0,), created_at=None,
                  ctr_start: int = 0, ctr_count: int = 1 << 32, epoch: int | None = None) -> MineRaceResult:
        """pow_mine_race: ``len(owners)`` rival miners race over `n` heights on
        top of `parent`; at every height the rival with the lowest solving
        counter wins (ties to the lowest position in `owners`) and its block is
        the next height's parent.  `created_at` has ``n * len(owners)`` entries,
        height-major.  ``blocks`` is the winners' chain tip first, a ctypes
        ``Block * n_mined`` array (what :meth:`verify_chain` takes), with
        ``winners`` and ``counters`` beside it; all are shorter than `n` if at
        some height no window held a solution or :meth:`cancel` was called
        meanwhile.  The host statement of the result is
        :func:`mpi_blockchain_amd.block.mine_race`."""
        R = len(owners)
        own = (ctypes.c_uint32 * max(R, 1))(*[o & 0xFFFFFFFF for o in owners])
        out = (Block * max(n, 1))()
        times = None
        if created_at is not None:
            if len(created_at) != n * R:
                raise ValueError(f"created_at has {len(created_at)} entries for {n} heights of {R} rivals")
            times = (ctypes.c_uint64 * max(n * R, 1))(*created_at)
        win = (ctypes.c_uint32 * max(n, 1))()
        ctrs = (ctypes.c_uint64 * max(n, 1))()
        mined, hashes = ctypes.c_size_t(), ctypes.c_uint64()
        ep = self._cancel.value if epoch is None else epoch
        rc = check(self.L.pow_mine_race(self.ctx, ctypes.byref(parent), n, difficulty, own, R, times, ctr_start,
                                        ctr_count, ctypes.byref(self._cancel), ep, out, win, ctrs,
                                        ctypes.byref(mined), ctypes.byref(hashes)), self.L)
        m = mined.value
        blocks = (Block * m)()
        if m:
            ctypes.memmove(blocks, ctypes.byref(out, (n - m) * ctypes.sizeof(Block)), m * ctypes.sizeof(Block))
        return MineRaceResult(blocks, list(win)[n - m:n], list(ctrs)[n - m:n], m, rc == 1, hashes.value,
                              self.stats()["kernel_ms"])

    def sweep(self, tmpl: Block, start: int, count: int, difficulty: int, cap: int | None = None) -> np.ndarray:
        """Ascending (counter - start) of every solving counter (count <= 2^32)."""
        if cap is None:  # pow_sweep sorts on the device: at most 2^31 - 1 entries
            cap = int(min(count, (count >> min(difficulty, 63)) * 2 + 4096, (1 << 31) - 1))
        out = np.zeros(max(cap, 1), dtype=np.uint32)
        n = ctypes.c_size_t()
        check(self.L.pow_sweep(self.ctx, ctypes.byref(tmpl), start, count, difficulty,
                               out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), cap, ctypes.byref(n)), self.L)
        return out[: n.value]  # a view: copying 33.6 MB (a 2^32 window at d = 9) again costs ~3 ms

    def sweep_count(self, tmpl: Block, start: int, count: int, difficulty: int,
                    dev_out=None, cap: int = 0) -> tuple[int, int | None]:
        """Count + lowest solving counter; the list (if any) stays on the GPU."""
        n, mn = ctypes.c_size_t(), ctypes.c_uint64()
        ptr = dev_out.ptr if isinstance(dev_out, DeviceBuffer) else dev_out
        check(self.L.pow_sweep_device(self.ctx, ctypes.byref(tmpl), start, count, difficulty,
                                      ptr if ptr else None, cap,
                                      ctypes.byref(n), ctypes.byref(mn)), self.L)
        return n.value, (None if mn.value == 0xFFFFFFFFFFFFFFFF else mn.value)


class StopBoard:
    """Cross-GPU stop board (include/pow_gpu.h): one slot per rank of a shared
    search, in host memory every GPU of the node maps.  name=None: private to
    this process; name="/x": POSIX shared memory, shared by every process of
    the node that opens it."""

    NONE = None

    def __init__(self, nslots: int, name: str | None = None, test_hooks: bool = False):
        self.L = load(test_hooks)
        self.name = name
        self.ptr = ctypes.c_void_p()
        check(self.L.pow_board_open(name.encode() if name else None, nslots, ctypes.byref(self.ptr)), self.L)

    def post(self, slot: int, tag: int, counter: int | None) -> None:
        check(self.L.pow_board_post(self.ptr, slot, tag, 0xFFFFFFFFFFFFFFFF if counter is None else counter), self.L)

    def peek(self, except_slot: int, tag: int) -> int | None:
        v = ctypes.c_uint64()
        check(self.L.pow_board_peek(self.ptr, except_slot, tag, ctypes.byref(v)), self.L)
        return None if v.value == 0xFFFFFFFFFFFFFFFF else v.value

    def unlink(self) -> None:
        if self.name:
            check(self.L.pow_board_unlink(self.name.encode()), self.L)

    def close(self) -> None:
        if self.ptr:
            self.L.pow_board_close(self.ptr)
            self.ptr = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class DeviceBuffer:
    """Device memory owned by a GpuMiner's context (raw pointer for the C ABI)."""

    def __init__(self, miner: "GpuMiner", nbytes: int):
        self.miner, self.nbytes = miner, nbytes
        self.ptr = ctypes.c_void_p()
        check(miner.L.pow_dev_alloc(miner.ctx, nbytes, ctypes.byref(self.ptr)), miner.L)

    def read_u32(self, n: int) -> np.ndarray:
        out = np.zeros(n, dtype=np.uint32)
        if n:
            check(self.miner.L.pow_dev_read(self.miner.ctx, self.ptr, out.ctypes.data_as(ctypes.c_void_p),
                                            4 * n), self.miner.L)
        return out

    def free(self) -> None:
        if self.ptr:
            check(self.miner.L.pow_dev_free(self.miner.ctx, self.ptr), self.miner.L)
            self.ptr = ctypes.c_void_p()


def proof_of_work_round(miner: GpuMiner, last: Block, rank: int, start: int, count: int,
                        difficulty: int = DEFAULT_DIFFICULTY) -> MineResult | None:
    """One round of node.cpp:285-308 on the GPU: template refresh, then the
    nonce -> hash -> test loop over a counter range."""
    return miner.mine(refresh_template(last, rank, difficulty), start, count, difficulty)


def replay_proof_of_work(miner: GpuMiner, last: Block, rank: int, seed: int, n_blocks: int,
                         difficulty: int = DEFAULT_DIFFICULTY, created_at=None) -> tuple[list, int]:
    """What a solo reference rank seeded ``srand(seed)`` does (node.cpp:285-318):
    refresh the template on the tip, test the stream's trials in order from
    where it stands, seal the first that solves, go on at the trial after it.
    created_at: one value per block (None: the clock, as the reference).
    Returns the blocks, oldest first, and the total trials the rank drew; fewer
    than `n_blocks` blocks if a 2^32 window held no solution."""
    blocks, at = [], 0
    for k in range(n_blocks):
        tmpl = refresh_template(last, rank, difficulty, None if created_at is None else created_at[k])
        r = miner.mine_rand(tmpl, seed, at, 1 << 32, difficulty)
        if r is None:
            break
        blocks.append(r.block)
        last, at = r.block, r.trial + 1
    return blocks, at


def audit_rand_provenance(miner: GpuMiner, chain, seed_window: tuple[int, int] | None = None,
                          count: int = 1 << 32) -> RandProvenance:
    """Were these blocks mined by reference ranks, and from which seeds?  The
    reference seeds with ``srand(time(NULL) + rank)`` (node.cpp:386) and keeps
    the seed nowhere, so it is recovered: one :meth:`GpuMiner.find_seed` over
    every block's nonce, trials [0, count) of every seed of the window.
    chain: at most 64 ``Block`` s, tip first.  seed_window: (first seed, number
    of seeds); None: from an hour before the earliest ``created_at`` to the
    latest plus the highest rank.  Nothing is raised on a failed verdict: they
    are all in the result (:class:`RandProvenance`)."""
    chain = list(chain)
    if not 1 <= len(chain) <= SEED_MAX_TARGETS:
        raise ValueError(f"a chain of 1 to {SEED_MAX_TARGETS} blocks")
    if seed_window is None:
        stamps = [b.created_at for b in chain]
        first = max(0, min(stamps) - 3600)
        seed_window = (first, max(stamps) + max(b.node_owner_number for b in chain) - first + 1)
    first, n_seeds = seed_window[0] & 0xFFFFFFFF, seed_window[1]
    if not 1 <= n_seeds <= SEED_MAX_SEEDS:
        raise ValueError(f"a window of {n_seeds} seeds (1 to {SEED_MAX_SEEDS})")
    nonces = [field(b, "nonce")[:NONCE_SIZE - 1] for b in chain]
    # a nonce with a byte outside the alphabet is not the generator's: searched for apart from the rest
    drawn = [k for k, n in enumerate(nonces) if len(n) == NONCE_SIZE - 1 and n.isalnum() and n.isascii()]
    found = miner.find_seed([nonces[k] for k in drawn], first, n_seeds, 0, count, cap=1 << 16) if drawn else []
    matches = [SeedMatch(m.seed, m.trial, drawn[m.target]) for m in found]
    pos = lambda seed: (seed - first) & 0xFFFFFFFF  # noqa: E731
    by_block: dict = {}
    for m in matches:  # block -> seed -> its lowest trial
        by_block.setdefault(m.target, {}).setdefault(m.seed, m.trial)
    rep = RandProvenance({}, [None] * len(chain), [k for k in range(len(chain)) if k not in by_block], {}, {}, {}, matches)
    for owner in sorted({b.node_owner_number for b in chain}):
        mine = [k for k, b in enumerate(chain) if b.node_owner_number == owner]
        cover: dict = {}
        for k in mine:
            for seed in by_block.get(k, {}):
                cover[seed] = cover.get(seed, 0) + 1
        seed = min(cover, key=lambda s: (-cover[s], pos(s))) if cover else None
        rep.seeds[owner] = seed
        rep.one_seed[owner] = seed is not None and cover[seed] == len(mine)
        rep.seed_in_window[owner] = seed is not None and pos(seed - owner) < n_seeds
        for k in mine:
            rep.trials[k] = by_block.get(k, {}).get(seed)
        order = [rep.trials[k] for k in sorted(mine, key=lambda k: chain[k].index)]
        rep.trials_increase[owner] = None not in order and all(a < b for a, b in zip(order, order[1:]))
    return rep


def block_hex(b: Block) -> str:
    return field(b, "block_hash").split(b"\0", 1)[0].decode()


__all__ = ["GpuMiner", "DeviceBuffer", "StopBoard", "MineResult", "MineRandResult", "rand_nonces", "replay_proof_of_work", "SeedMatch", "RandProvenance", "audit_rand_provenance", "MineChainResult", "MineBatchResult", "VerifyResult", "VerifyChainsResult", "refresh_template", "proof_of_work_round", "block_hex",
           "nonce_from_counter"]
