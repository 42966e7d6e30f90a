"""ctypes binding of ``libpow_gpu.so`` (include/pow_gpu.h, include/pow_tools.h).

There is deliberately NO fallback: if the native library is missing or fails
to load, this raises.  The product path never routes through a CPU
implementation (the CPU checkers live in ``oracle/`` and are test-only).
"""
from __future__ import annotations

import ctypes
import os

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG, "libpow_gpu.so")
# The same objects plus csrc/pow_hooks.cpp (build.py TEST_ONLY): test and tuning
# switches read from the environment at pow_init.  Only tests load it.
TEST_LIB_PATH = os.path.join(PKG, "libpow_gpu_test.so")

HASH_SIZE = 256
NONCE_SIZE = 10
MSG_BYTES = 270
COUNTER_LIMIT = 62**9
RAND_TRIAL_LIMIT = 1 << 56
SEED_MAX_SEEDS, SEED_MAX_TARGETS = 1 << 20, 64

POW_OK, POW_EINVAL, POW_ENOSPC, POW_EHIP, POW_ENODEV, POW_ECOMM = 0, -1, -2, -3, -4, -5
_ERRNAMES = {POW_EINVAL: "POW_EINVAL", POW_ENOSPC: "POW_ENOSPC", POW_EHIP: "POW_EHIP",
             POW_ENODEV: "POW_ENODEV", POW_ECOMM: "POW_ECOMM"}
GROUP_ID_BYTES = 128
BOARD_MAX_SLOTS, BOARD_MAX_TAG = 64, 1023
POW_REDUCE_MIN, POW_REDUCE_MAX, POW_REDUCE_SUM = 0, 1, 2
POW_V_HASH, POW_V_WORK, POW_V_LINK, POW_V_INDEX = 1, 2, 4, 8
POOL_MAX_BLOCKS, POOL_ROOT, POOL_NONE = 1 << 20, 0xFFFFFFFF, 0xFFFFFFFE


class PowError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{_ERRNAMES.get(code, code)}: {msg}")
        self.code = code


class Block(ctypes.Structure):
    """``struct Block`` of block.h:17-25 (== ``pow_block``), sizeof 552."""

    _fields_ = [
        ("index", ctypes.c_uint32),
        ("node_owner_number", ctypes.c_uint32),
        ("difficulty", ctypes.c_uint32),
        ("created_at", ctypes.c_uint64),
        ("nonce", ctypes.c_char * NONCE_SIZE),
        ("previous_block_hash", ctypes.c_char * HASH_SIZE),
        ("block_hash", ctypes.c_char * HASH_SIZE),
    ]


# int reduce(void* user, uint64_t* vals, size_t n, int op): pow_group_reduce_fn
REDUCE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_size_t,
                             ctypes.c_int)


class PowStats(ctypes.Structure):
    _fields_ = [("kernel_ms", ctypes.c_double), ("launches", ctypes.c_uint32),
                ("hashes", ctypes.c_uint64)]


class SeedMatchRec(ctypes.Structure):
    """pow_seed_match (include/pow_gpu.h): one match of pow_find_seed."""

    _fields_ = [("seed", ctypes.c_uint32), ("target", ctypes.c_uint32), ("trial", ctypes.c_uint64)]


class ValuResult(ctypes.Structure):
    """pow_valu_result (include/pow_tools.h)."""

    _fields_ = [("lane_ops_per_s", ctypes.c_double), ("kernel_ms", ctypes.c_double),
                ("clock_hz", ctypes.c_double), ("cycles_per_instr", ctypes.c_double)]


class GroupSearchInfo(ctypes.Structure):
    """pow_group_search_info (include/pow_gpu.h): this rank's part in the
    group's last search."""

    _fields_ = [("board_open", ctypes.c_int), ("board_bound", ctypes.c_int), ("rounds", ctypes.c_uint32),
                ("local_found", ctypes.c_int), ("mine_end_ns", ctypes.c_uint64), ("mine_ms", ctypes.c_double),
                ("allreduce_ms", ctypes.c_double)]


class PoolInfo(ctypes.Structure):
    """pow_pool_info (include/pow_gpu.h): a pow_pool after its last add or prune."""

    _fields_ = [(n, ctypes.c_uint32) for n in ("size", "n_flagged", "best", "best_index", "adopted", "reranked",
                                               "rehashed", "capacity", "slots")]


class PoolLiftInfo(ctypes.Structure):
    """pow_pool_lift_info (include/pow_gpu.h): the binary-lifting table of a pow_pool's ancestry queries."""

    _fields_ = [(n, ctypes.c_uint32) for n in ("covered", "rows", "capacity", "rebuilt", "extended")] + \
               [("bytes", ctypes.c_uint64)]


POW_KEEP_BY_INDEX, POW_KEEP_SOUND_ONLY, POOL_MAX_TIPS = 1, 2, 1 << 16  # pow_pool_mark, pow_pool_prune
POW_TIPS_SOUND_ONLY, POOL_MAX_ROOTS = 1, 64  # pow_pool_tips; pow_pool_subtrees, pow_pool_drop
POW_VALU_MIX, POW_VALU_FULL, POW_VALU_HALF = 0, 1, 2
POW_LAUNCH_HIP, POW_LAUNCH_DIRECT = 0, 1

assert ctypes.sizeof(Block) == 552

_libs: dict = {}


def load(test_hooks: bool = False) -> ctypes.CDLL:
    """Load libpow_gpu.so (raises if it is missing — no fallback).
    test_hooks=True: libpow_gpu_test.so, the same code plus the test switches
    (tests only; both may be loaded in one process, each with its own handle)."""
    path = TEST_LIB_PATH if test_hooks else LIB_PATH
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: build it with `python -m mpi_blockchain_amd.build` "
            "(the GPU path has no CPU fallback)")
    # One HIP runtime per process: when PyTorch-ROCm is importable, load it
    # first so this library binds to the same libamdhip64.so.7 (same soname).
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is optional for the C ABI
        pass
    L = ctypes.CDLL(path)
    P = ctypes.POINTER(Block)
    c_u64p = ctypes.POINTER(ctypes.c_uint64)
    c_sizep = ctypes.POINTER(ctypes.c_size_t)
    sigs = {
        "pow_device_count": ([ctypes.POINTER(ctypes.c_int)], ctypes.c_int),
        "pow_init": ([ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)], ctypes.c_int),
        "pow_destroy": ([ctypes.c_void_p], None),
        "pow_warmup": ([ctypes.c_void_p], ctypes.c_int),
        "pow_last_error": ([], ctypes.c_char_p),
        "pow_get_stats": ([ctypes.c_void_p, ctypes.POINTER(PowStats)], ctypes.c_int),
        "pow_launch_path": ([ctypes.c_void_p], ctypes.c_int),
        "pow_device_pci_bus_id": ([ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t], ctypes.c_int),
        "pow_device_info": ([ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                             ctypes.c_char_p, ctypes.c_size_t], ctypes.c_int),
        "pow_nonce_from_counter": ([ctypes.c_uint64, ctypes.c_char_p], ctypes.c_int),
        "pow_block_to_bytes": ([P, ctypes.c_char_p], ctypes.c_int),
        "pow_solves_problem": ([ctypes.c_char_p, ctypes.c_uint], ctypes.c_int),
        "pow_rand_nonces": ([ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_char_p], ctypes.c_int),
        "pow_mine_rand": ([ctypes.c_void_p, P, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint,
                           ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32, P, c_u64p, c_u64p], ctypes.c_int),
        "pow_find_seed": ([ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32,
                           ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32,
                           ctypes.POINTER(SeedMatchRec), ctypes.c_size_t, c_sizep, c_u64p], ctypes.c_int),
        "pow_hash_blocks": ([ctypes.c_void_p, P, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_char_p],
                            ctypes.c_int),
        "pow_hash_block": ([ctypes.c_void_p, P, ctypes.c_char_p, ctypes.c_char_p], ctypes.c_int),
        "pow_verify_chain": ([ctypes.c_void_p, P, ctypes.c_size_t, ctypes.c_uint, ctypes.c_void_p, c_sizep, c_sizep],
                             ctypes.c_int),
        "pow_verify_chains": ([ctypes.c_void_p, P, ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t, ctypes.c_uint,
                               ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32),
                               c_sizep], ctypes.c_int),
        "pow_index_blocks": ([ctypes.c_void_p, P, ctypes.c_size_t, ctypes.c_uint, ctypes.c_void_p,
                              ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32),
                              ctypes.POINTER(ctypes.c_uint32), c_sizep], ctypes.c_int),
        "pow_pool_open": ([ctypes.c_void_p, ctypes.c_uint, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)],
                          ctypes.c_int),
        "pow_pool_close": ([ctypes.c_void_p], None),
        "pow_pool_add": ([ctypes.c_void_p, P, ctypes.c_size_t, ctypes.POINTER(PoolInfo)], ctypes.c_int),
        "pow_pool_get_info": ([ctypes.c_void_p, ctypes.POINTER(PoolInfo)], ctypes.c_int),
        "pow_pool_read": ([ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p,
                           ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32),
                           ctypes.POINTER(ctypes.c_uint32)], ctypes.c_int),
        "pow_pool_find": ([ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32)],
                          ctypes.c_int),
        "pow_pool_mark": ([ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t, ctypes.c_uint32,
                           ctypes.c_uint, ctypes.c_void_p, c_sizep], ctypes.c_int),
        "pow_pool_prune": ([ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t, ctypes.c_uint32,
                            ctypes.c_uint, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(PoolInfo)], ctypes.c_int),
        "pow_pool_ancestors": ([ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32),
                                ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32)], ctypes.c_int),
        "pow_pool_fork_points": ([ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32),
                                  ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32),
                                  ctypes.POINTER(ctypes.c_uint32)], ctypes.c_int),
        "pow_pool_chain": ([ctypes.c_void_p, ctypes.c_uint32, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32),
                            c_sizep], ctypes.c_int),
        "pow_pool_lift_get_info": ([ctypes.c_void_p, ctypes.POINTER(PoolLiftInfo)], ctypes.c_int),
        "pow_pool_tips": ([ctypes.c_void_p, ctypes.c_uint, ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t, c_sizep],
                          ctypes.c_int),
        "pow_pool_subtrees": ([ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t,
                               ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32),
                               ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32), ctypes.c_void_p,
                               c_sizep], ctypes.c_int),
        "pow_pool_drop": ([ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t,
                           ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(PoolInfo)], ctypes.c_int),
        "pow_mine_chain": ([ctypes.c_void_p, P, ctypes.c_size_t, ctypes.c_uint, ctypes.c_uint32, c_u64p,
                            ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32, P,
                            c_sizep, c_u64p], ctypes.c_int),
        "pow_mine_batch": ([ctypes.c_void_p, P, ctypes.c_size_t, ctypes.c_uint, ctypes.c_uint64, ctypes.c_uint64,
                            ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32, P, c_u64p, c_sizep, c_u64p], ctypes.c_int),
        "pow_mine_race": ([ctypes.c_void_p, P, ctypes.c_size_t, ctypes.c_uint, ctypes.POINTER(ctypes.c_uint32),
                           ctypes.c_size_t, c_u64p, ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint32),
                           ctypes.c_uint32, P, ctypes.POINTER(ctypes.c_uint32), c_u64p, c_sizep, c_u64p], ctypes.c_int),
        "pow_mine": ([ctypes.c_void_p, P, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint,
                      ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32, P, c_u64p, c_u64p], ctypes.c_int),
        "pow_mine_any": ([ctypes.c_void_p, P, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint,
                          ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32, P, c_u64p, c_u64p], ctypes.c_int),
        "pow_sweep": ([ctypes.c_void_p, P, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint,
                       ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t, c_sizep], ctypes.c_int),
        "pow_sweep_device": ([ctypes.c_void_p, P, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint,
                              ctypes.c_void_p, ctypes.c_size_t, c_sizep, c_u64p], ctypes.c_int),
        "pow_cancel": ([ctypes.c_void_p, ctypes.c_uint32], ctypes.c_int),
        "pow_dev_alloc": ([ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)], ctypes.c_int),
        "pow_dev_free": ([ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int),
        "pow_dev_read": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t], ctypes.c_int),
        "pow_group_partition": ([ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, c_u64p, c_u64p],
                                None),
        "pow_group_unique_id": ([ctypes.c_char_p], ctypes.c_int),
        "pow_group_init": ([ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_char_p,
                            ctypes.POINTER(ctypes.c_void_p)], ctypes.c_int),
        "pow_group_init_within": ([ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_uint,
                                   ctypes.POINTER(ctypes.c_void_p)], ctypes.c_int),
        "pow_group_init_custom": ([ctypes.c_void_p, ctypes.c_int, ctypes.c_int, REDUCE_FN, ctypes.c_void_p,
                                   ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p)], ctypes.c_int),
        "pow_group_destroy": ([ctypes.c_void_p], None),
        "pow_group_info": ([ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)], ctypes.c_int),
        "pow_group_rccl_path": ([ctypes.c_char_p, ctypes.c_size_t], ctypes.c_int),
        "pow_group_last_search": ([ctypes.c_void_p, ctypes.POINTER(GroupSearchInfo)], ctypes.c_int),
        "pow_group_allreduce_u64": ([ctypes.c_void_p, c_u64p, ctypes.c_size_t, ctypes.c_int], ctypes.c_int),
        "pow_group_mine": ([ctypes.c_void_p, P, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint,
                            ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32, P, c_u64p, c_u64p], ctypes.c_int),
        "pow_group_mine_any": ([ctypes.c_void_p, P, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint,
                                ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32, P, c_u64p, c_u64p], ctypes.c_int),
        "pow_board_open": ([ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)], ctypes.c_int),
        "pow_board_unlink": ([ctypes.c_char_p], ctypes.c_int),
        "pow_board_close": ([ctypes.c_void_p], None),
        "pow_board_bind": ([ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32], ctypes.c_int),
        "pow_board_post": ([ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64], ctypes.c_int),
        "pow_board_peek": ([ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, c_u64p], ctypes.c_int),
        "pow_valu_peak": ([ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)],
                          ctypes.c_int),
        "pow_valu_rate": ([ctypes.c_int, ctypes.c_int, ctypes.POINTER(ValuResult)], ctypes.c_int),
        "pow_valu_rate_ctx": ([ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ValuResult)], ctypes.c_int),
    }
    for name, (args, res) in sigs.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = res
    _libs[path] = L
    return L


EXPORTS = ("pow_device_count", "pow_init", "pow_warmup", "pow_destroy", "pow_last_error", "pow_get_stats", "pow_launch_path",
           "pow_device_info", "pow_device_pci_bus_id",
           "pow_nonce_from_counter", "pow_block_to_bytes", "pow_solves_problem", "pow_hash_blocks",
           "pow_hash_block", "pow_verify_chain", "pow_verify_chains", "pow_index_blocks", "pow_pool_open", "pow_pool_close", "pow_pool_add", "pow_pool_get_info", "pow_pool_read", "pow_pool_find", "pow_pool_mark", "pow_pool_prune", "pow_pool_ancestors", "pow_pool_fork_points", "pow_pool_chain", "pow_pool_lift_get_info", "pow_pool_tips", "pow_pool_subtrees", "pow_pool_drop", "pow_mine_chain", "pow_mine_batch", "pow_mine_race", "pow_mine_rand", "pow_rand_nonces", "pow_find_seed", "pow_mine", "pow_mine_any", "pow_cancel", "pow_sweep", "pow_sweep_device", "pow_dev_alloc", "pow_dev_free",
           "pow_dev_read", "pow_valu_peak", "pow_valu_rate", "pow_valu_rate_ctx", "pow_group_partition", "pow_group_unique_id", "pow_group_init",
           "pow_group_init_within",
           "pow_group_init_custom", "pow_group_destroy", "pow_group_info", "pow_group_rccl_path", "pow_group_last_search",
           "pow_group_allreduce_u64", "pow_group_mine", "pow_group_mine_any",
           "pow_board_open", "pow_board_unlink", "pow_board_close", "pow_board_bind", "pow_board_post",
           "pow_board_peek")


def check(rc: int, L: ctypes.CDLL | None = None) -> int:
    """Raise PowError for rc < 0 with the message of the library that failed
    (each loaded library keeps its own pow_last_error)."""
    if rc < 0:
        raise PowError(rc, ((L or load()).pow_last_error() or b"").decode(errors="replace"))
    return rc
