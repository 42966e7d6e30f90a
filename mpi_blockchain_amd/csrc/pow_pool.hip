// K10  the kernels of pow_index_blocks: the block tree of a pool of raw
// structs in any order, the audit of every chain in it and the fork choice.
// The reference walks map<string,Block> node_blocks by previous_block_hash
// (sanity_test, verify_chain_indexes, look_for_block: node.cpp:40-148); here a
// block's name is its computed digest, its parent is found through a hash
// table of pool positions, and every walk is ranked at once.
//
//   K10a pow_pool_audit_kernel   per host tile, K3's frame: one lane per block,
//        one wave per workgroup, 64 raw structs in LDS (no halo: nobody's
//        parent is its neighbour).  Per block: POW_V_HASH | POW_V_WORK
//        (pow_audit_dev.h), the digest, the index field and the parsed
//        previous_block_hash (eight words and a kind).
//   K10b pow_pool_insert_kernel  the named blocks (not POW_V_HASH) into an
//        open-addressed table of pool positions.
//   K10c pow_pool_join_kernel    every block's parent by its parsed name;
//        POW_V_LINK, POW_V_INDEX; the ranking's first state.
//   K10d pow_pool_round_kernel   one round of pointer jumping, ping-pong.
//   K10e pow_pool_finish_kernel  what a walk that never ended gets, the count
//        of flagged blocks and the fork choice.
//
// Memory ordering of K10b.  The digests were written by earlier launches
// (K10a), so plain loads read them.  The only thing handed from lane to lane
// inside the launch is a slot's word, and only through atomics (atomicCAS from
// empty, atomicMin among equal digests): a slot never changes from one digest
// to another, so what a lane learns from the position it read out of a slot
// (that position's digest) stays true whatever the slot holds later.  No fence
// is needed.  K10c runs in a later launch and reads the table with plain loads.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pow_audit_dev.h"
#include "pow_ctx.h"
#include "pow_pool_dev.h"  // SLOT_EMPTY, unhex4, same_digest: shared with K11 (pow_pool_live.hip)

using namespace powaudit;

// blocks: the n_check structs of a host tile; base: the pool position of its
// first.  K3's budget: at most 64 VGPRs, no scratch, the LDS of the tile only.
__global__ __launch_bounds__(64) __attribute__((amdgpu_num_vgpr(64))) void pow_pool_audit_kernel(
    const uint32_t* __restrict__ blocks, uint32_t n_check, uint32_t base, uint32_t diff, uint8_t* __restrict__ status,
    uint8_t* __restrict__ kind, uint4* __restrict__ dig, uint4* __restrict__ prev, uint32_t* __restrict__ index) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[TILE * BLK_DW];
  const uint32_t lane = threadIdx.x;
  const uint32_t first = blockIdx.x * TILE;
  load_tile(lds, blocks, first, min(n_check, first + TILE), lane);  // at most TILE blocks: no halo
  __syncthreads();
  const uint32_t t = first + lane;
  if (t >= n_check) return;
  const uint32_t* const b = lds + lane * BLK_DW;
  uint32_t h[8];
  hash_block(b, h);
  const uint32_t flags = own_flags(b, h, diff);
  // previous_block_hash, struct byte 34: two bytes past dword 8, as block_hash
  // is two past dword 72.  A digest's name is 64 characters of 0-9a-f and a NUL
  // at byte 98 (dword 24, byte 2); a NUL at byte 34 is the empty string.
  uint32_t p[8], bad = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint32_t d0 = b[8 + 2 * k], d1 = b[9 + 2 * k], d2 = b[10 + 2 * k];
    const uint32_t hi = unhex4((d0 >> 16) | (d1 << 16), bad);
    p[k] = (hi << 16) | unhex4((d1 >> 16) | (d2 << 16), bad);
  }
  bad |= b[24] & 0x00FF0000u;
  const uint32_t g = base + t;
  status[g] = (uint8_t)flags;
  kind[g] = (uint8_t)((b[8] & 0x00FF0000u) == 0u ? POW_PREV_EMPTY : bad ? POW_PREV_UNMATCHABLE : POW_PREV_DIGEST);
  index[g] = b[0];
  dig[2u * g] = make_uint4(h[0], h[1], h[2], h[3]);
  dig[2u * g + 1u] = make_uint4(h[4], h[5], h[6], h[7]);
  prev[2u * g] = make_uint4(p[0], p[1], p[2], p[3]);
  prev[2u * g + 1u] = make_uint4(p[4], p[5], p[6], p[7]);
}

// table: mask + 1 slots, all SLOT_EMPTY.  A named block probes linearly from
// the slot its last digest word names (under difficulty d the first word's
// leading d bits are zero).  atomicCAS from empty takes a slot; a slot that
// holds a block of the same digest keeps the lowest position of them
// (atomicMin: std::map::insert keeps what came first); a slot of another
// digest is passed.  A CAS that fails returns who holds the slot, and that
// same slot is judged by it.  The loop ends after mask + 1 probes: a lane that
// found no slot sets ctl->err and the call fails; nobody spins.
__global__ __launch_bounds__(256) void pow_pool_insert_kernel(const uint8_t* __restrict__ status,
                                                              const uint4* __restrict__ dig, uint32_t* table,
                                                              uint32_t n, uint32_t mask, PowPoolCtl* ctl) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n || (status[i] & POW_V_HASH)) return;
  const uint4 a = dig[2u * i], b = dig[2u * i + 1u];
  uint32_t slot = b.w & mask;
  for (uint32_t probe = 0; probe <= mask; ++probe) {
    const uint32_t held = atomicCAS(&table[slot], SLOT_EMPTY, i);
    if (held == SLOT_EMPTY) return;
    if (held >= n) break;  // not a position of this pool: the table was not reset
    if (same_digest(dig, held, a, b)) {
      atomicMin(&table[slot], i);
      return;
    }
    slot = (slot + 1u) & mask;
  }
  atomicOr(&ctl->err, 1u);
}

// Every block's parent: POW_POOL_ROOT for an empty previous_block_hash,
// the named block of that digest, POW_POOL_NONE if there is none or the field
// can name nobody.  The probe ends at an equal digest or an empty slot, or
// after mask + 1 slots.  Then the flags against the parent, and the ranking's
// first state: next = parent, depth = 1, bad = flagged.
__global__ __launch_bounds__(256) void pow_pool_join_kernel(uint8_t* __restrict__ status,
                                                            const uint8_t* __restrict__ kind,
                                                            const uint4* __restrict__ dig,
                                                            const uint4* __restrict__ prev,
                                                            const uint32_t* __restrict__ index,
                                                            const uint32_t* __restrict__ table, uint32_t n,
                                                            uint32_t mask, uint32_t* __restrict__ parent,
                                                            uint32_t* __restrict__ next, uint32_t* __restrict__ depth,
                                                            uint32_t* __restrict__ bad) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  uint32_t flags = status[i];
  const uint32_t k = kind[i];
  uint32_t par = k == POW_PREV_EMPTY ? POW_POOL_ROOT : POW_POOL_NONE;
  if (k == POW_PREV_DIGEST) {
    const uint4 a = prev[2u * i], b = prev[2u * i + 1u];
    uint32_t slot = b.w & mask;
    for (uint32_t probe = 0; probe <= mask; ++probe) {
      const uint32_t held = table[slot];
      if (held >= n) break;  // empty: the pool holds no block of that name
      if (same_digest(dig, held, a, b)) {
        par = held;
        break;
      }
      slot = (slot + 1u) & mask;
    }
  }
  if (par == POW_POOL_NONE) flags |= POW_V_LINK;
  else if (par != POW_POOL_ROOT && index[i] - 1u != index[par]) flags |= POW_V_INDEX;
  status[i] = (uint8_t)flags;
  parent[i] = par;
  next[i] = par;
  depth[i] = 1u;
  bad[i] = flags != 0u ? 1u : 0u;
}

// One round of pointer jumping from the buffers `a` into the buffers `b`: a
// walk that has not ended (next < n) takes over what its next has gathered and
// jumps to that one's next; one that has ended (POW_POOL_ROOT, POW_POOL_NONE)
// stays as it is.  After r rounds next is 2^r steps along, depth and bad count
// the blocks in between.
__global__ __launch_bounds__(256) void pow_pool_round_kernel(uint32_t n, const uint32_t* __restrict__ next_a,
                                                             const uint32_t* __restrict__ depth_a,
                                                             const uint32_t* __restrict__ bad_a,
                                                             uint32_t* __restrict__ next_b,
                                                             uint32_t* __restrict__ depth_b,
                                                             uint32_t* __restrict__ bad_b) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  uint32_t nx = next_a[i], d = depth_a[i], f = bad_a[i];
  if (nx < n) {
    d += depth_a[nx];
    f += bad_a[nx];
    nx = next_a[nx];
  }
  next_b[i] = nx;
  depth_b[i] = d;
  bad_b[i] = f;
}

// After the rounds.  A walk that has still not ended lies on or above a cycle:
// depth 0, n_bad all ones, POW_V_LINK.  Then, one atomic of each kind per wave
// that needs it: the flagged blocks are counted, and among the blocks with
// n_bad == 0 the greatest (index << 32 | ~position) is kept: the highest index,
// the lowest position on a tie.  A key is never 0 (a position is below 2^20).
__global__ __launch_bounds__(256) void pow_pool_finish_kernel(uint32_t n, const uint32_t* __restrict__ next,
                                                              uint32_t* __restrict__ depth, uint32_t* __restrict__ bad,
                                                              uint8_t* __restrict__ status,
                                                              const uint32_t* __restrict__ index, PowPoolCtl* ctl) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  unsigned long long key = 0ull;
  bool flagged = false;
  if (i < n) {
    uint32_t st = status[i];
    if (next[i] < n) {
      depth[i] = 0u;
      bad[i] = 0xFFFFFFFFu;
      st |= POW_V_LINK;
      status[i] = (uint8_t)st;
    } else if (bad[i] == 0u) {
      key = ((unsigned long long)index[i] << 32) | (uint32_t)~i;
    }
    flagged = st != 0u;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)key, off);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(key >> 32), off);
    const unsigned long long other = ((unsigned long long)hi << 32) | lo;
    key = other > key ? other : key;
  }
  const unsigned long long any = __ballot(flagged);
  if ((threadIdx.x & 63u) == 0u) {
    if (key) atomicMax(&ctl->best, key);
    if (any) atomicAdd(&ctl->n_flagged, (uint32_t)__builtin_popcountll(any));
  }
}

hipError_t pow_launch_pool_audit(hipStream_t stream, const uint32_t* blocks, uint32_t n_check, uint32_t base,
                                 unsigned diff, const PowPoolDev& D) {
  if (n_check == 0) return hipSuccess;
  hipLaunchKernelGGL(pow_pool_audit_kernel, dim3((n_check + TILE - 1) / TILE), dim3(TILE), 0, stream, blocks, n_check,
                     base, (uint32_t)diff, D.status, D.kind, (uint4*)D.dig, (uint4*)D.prev, D.index);
  return hipGetLastError();
}

hipError_t pow_launch_pool_insert(hipStream_t stream, const PowPoolDev& D) {
  hipLaunchKernelGGL(pow_pool_insert_kernel, dim3((D.n + 255u) / 256u), dim3(256), 0, stream, D.status,
                     (const uint4*)D.dig, D.table, D.n, D.slots - 1u, D.ctl);
  return hipGetLastError();
}

hipError_t pow_launch_pool_join(hipStream_t stream, const PowPoolDev& D) {
  hipLaunchKernelGGL(pow_pool_join_kernel, dim3((D.n + 255u) / 256u), dim3(256), 0, stream, D.status, D.kind,
                     (const uint4*)D.dig, (const uint4*)D.prev, D.index, D.table, D.n, D.slots - 1u, D.parent,
                     D.next[0], D.depth[0], D.bad[0]);
  return hipGetLastError();
}

// Round r reads the buffers r & 1 and writes the others.
hipError_t pow_launch_pool_round(hipStream_t stream, const PowPoolDev& D, uint32_t r) {
  const uint32_t a = r & 1u, b = a ^ 1u;
  hipLaunchKernelGGL(pow_pool_round_kernel, dim3((D.n + 255u) / 256u), dim3(256), 0, stream, D.n, D.next[a],
                     D.depth[a], D.bad[a], D.next[b], D.depth[b], D.bad[b]);
  return hipGetLastError();
}

// which: the buffers the last round wrote (rounds & 1).
hipError_t pow_launch_pool_finish(hipStream_t stream, const PowPoolDev& D, uint32_t which) {
  hipLaunchKernelGGL(pow_pool_finish_kernel, dim3((D.n + 255u) / 256u), dim3(256), 0, stream, D.n, D.next[which],
                     D.depth[which], D.bad[which], D.status, D.index, D.ctl);
  return hipGetLastError();
}
