// K11  the kernels of pow_pool_add and pow_pool_find: K10's block tree kept on
// the device and fed in batches.  The pool holds n blocks after the add, of
// which the positions below `base` were there before it (the old blocks) and
// base..n-1 came with it (the new ones).  K10a audits the new blocks as it
// stands (pow_pool.hip), and an add that has to rebuild the table or to
// re-rank the whole pool does so with K10b to K10e as they stand.
//
//   K11b pow_pool_live_insert_kernel  K10b over the new blocks only.
//   K11c pow_pool_live_join_kernel    one lane per block of the pool.  A new
//        block is joined as K10c joins it.  An old block does work only if it
//        is an orphan whose previous_block_hash can name somebody (parent
//        POW_POOL_NONE, kind POW_PREV_DIGEST): it probes the table, and if its
//        parent has arrived it counts itself in ctl->adopted and writes
//        nothing.  Nothing else about an old block can change: a new twin of a
//        named block has a higher position and never takes the name over.
//   K11d pow_pool_live_round_kernel   K10d over the new blocks: a walk jumps
//        only while its next is a new block, so it ends at a root, at
//        POW_POOL_NONE or at an old block after ceil(log2 m) rounds.
//   K11e pow_pool_live_finish_kernel  a walk that ended at an old block takes
//        over that block's final depth and n_bad; the new blocks feed the
//        resident fork choice and flagged count, which the old blocks' part
//        of stands as it is.
//   K11s pow_pool_live_strip_kernel   before a re-rank: every status back to
//        POW_V_HASH | POW_V_WORK, what K10a wrote.
//   K11f pow_pool_live_find_kernel    pow_pool_find: a name's 64 characters
//        parsed as K10a parses previous_block_hash, and K10c's probe.
//
// Memory ordering of K11b: K10b's (pow_pool.hip).  The new blocks' digests were
// written by an earlier launch (K10a), the old blocks' by earlier calls; a
// slot's word is handed from lane to lane through atomics only and never
// changes from one digest to another.  The slots the old blocks hold are read
// by the same atomics that would take them.  K11c runs in a later launch and
// reads the table with plain loads.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pow_ctx.h"
#include "pow_pool_dev.h"

// K10b over the positions base..n-1: the same atomics, the same bounded probe.
__global__ __launch_bounds__(256) void pow_pool_live_insert_kernel(const uint8_t* __restrict__ status,
                                                                   const uint4* __restrict__ dig, uint32_t* table,
                                                                   uint32_t base, uint32_t n, uint32_t mask,
                                                                   PowPoolCtl* ctl) {
  const uint32_t i = base + blockIdx.x * 256u + threadIdx.x;
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

// One lane per block of the pool.  New blocks (i >= base): K10c.  Old blocks:
// the scan for adopted orphans, 4 bytes read per block and no write; one
// atomic per wave that has found one.
__global__ __launch_bounds__(256) void pow_pool_live_join_kernel(uint8_t* status, const uint8_t* __restrict__ kind,
                                                                 const uint4* __restrict__ dig,
                                                                 const uint4* __restrict__ prev,
                                                                 const uint32_t* __restrict__ index,
                                                                 const uint32_t* __restrict__ table, uint32_t base,
                                                                 uint32_t n, uint32_t mask, uint32_t* parent,
                                                                 uint32_t* next, uint32_t* depth, uint32_t* bad,
                                                                 PowPoolLiveCtl* ctl) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const bool fresh = i >= base;
  bool adopted = false;
  if (i < n) {
    uint32_t par = POW_POOL_NONE;
    bool look = fresh;
    if (!fresh) look = parent[i] == POW_POOL_NONE;  // an orphan so far
    if (look) {
      const uint32_t k = kind[i];
      if (k == POW_PREV_EMPTY && fresh) par = POW_POOL_ROOT;  // an old root is no orphan and does not get here
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
    }
    if (fresh) {
      uint32_t flags = status[i];
      if (par == POW_POOL_NONE) flags |= POW_V_LINK;
      else if (par != POW_POOL_ROOT && index[i] - 1u != index[par]) flags |= POW_V_INDEX;
      status[i] = (uint8_t)flags;
      parent[i] = par;
      next[i] = par;
      depth[i] = 1u;
      bad[i] = flags != 0u ? 1u : 0u;
    } else {
      adopted = par != POW_POOL_NONE;
    }
  }
  const unsigned long long any = __ballot(adopted);
  if ((threadIdx.x & 63u) == 0u && any) atomicAdd(&ctl->adopted, (uint32_t)__builtin_popcountll(any));
}

// K10d over the positions base..n-1; a walk stays where it is once its next is
// not a new block.
__global__ __launch_bounds__(256) void pow_pool_live_round_kernel(uint32_t base, uint32_t n,
                                                                  const uint32_t* __restrict__ next_a,
                                                                  const uint32_t* __restrict__ depth_a,
                                                                  const uint32_t* __restrict__ bad_a,
                                                                  uint32_t* __restrict__ next_b,
                                                                  uint32_t* __restrict__ depth_b,
                                                                  uint32_t* __restrict__ bad_b) {
  const uint32_t i = base + blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  uint32_t nx = next_a[i], d = depth_a[i], f = bad_a[i];
  if (nx - base < n - base) {
    d += depth_a[nx];
    f += bad_a[nx];
    nx = next_a[nx];
  }
  next_b[i] = nx;
  depth_b[i] = d;
  bad_b[i] = f;
}

// After the rounds, over the positions base..n-1.  next, depth_w, bad_w: what
// the last round wrote.  depth_fin, bad_fin: the pool's final arrays, which
// hold the old blocks' values and take the new ones (they may be depth_w and
// bad_w themselves: a lane writes its own entry and reads old blocks' only).
// A walk that ended at an old block adds that block's depth and n_bad; one
// that never ended, or ended at a block that never ends, gets K10e's depth 0,
// n_bad all ones and POW_V_LINK.  Then K10e's two atomics per wave, into words
// that the earlier adds have fed: the key only grows and the count only adds.
__global__ __launch_bounds__(256) void pow_pool_live_finish_kernel(uint32_t base, uint32_t n,
                                                                   const uint32_t* __restrict__ next,
                                                                   const uint32_t* depth_w, const uint32_t* bad_w,
                                                                   uint32_t* depth_fin, uint32_t* bad_fin,
                                                                   uint8_t* __restrict__ status,
                                                                   const uint32_t* __restrict__ index,
                                                                   PowPoolCtl* ctl) {
  const uint32_t i = base + blockIdx.x * 256u + threadIdx.x;
  unsigned long long key = 0ull;
  bool flagged = false;
  if (i < n) {
    uint32_t st = status[i];
    const uint32_t nx = next[i];
    uint32_t d = depth_w[i], f = bad_w[i];
    bool open = nx - base < n - base;
    if (!open && nx < base) {
      const uint32_t under = bad_fin[nx];
      open = under == 0xFFFFFFFFu;
      d += depth_fin[nx];
      f += under;
    }
    if (open) {
      d = 0u;
      f = 0xFFFFFFFFu;
      st |= POW_V_LINK;
      status[i] = (uint8_t)st;
    }
    depth_fin[i] = d;
    bad_fin[i] = f;
    if (f == 0u) key = ((unsigned long long)index[i] << 32) | (uint32_t)~i;
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

// Four status bytes per lane back to what K10a wrote; words = ceil(n / 4), all
// inside the array (its capacity is whole words).
__global__ __launch_bounds__(256) void pow_pool_live_strip_kernel(uint32_t* __restrict__ status4, uint32_t words) {
  const uint32_t w = blockIdx.x * 256u + threadIdx.x;
  if (w < words) status4[w] &= (uint32_t)(POW_V_HASH | POW_V_WORK) * 0x01010101u;
}

// names: k x 64 characters on 16 bytes.  A name of 64 characters of 0-9a-f
// finds the named block of that digest (the slot holds the lowest position of
// its twins), anything else POW_POOL_NONE.
__global__ __launch_bounds__(256) void pow_pool_live_find_kernel(const uint4* __restrict__ names, uint32_t k,
                                                                 const uint4* __restrict__ dig,
                                                                 const uint32_t* __restrict__ table, uint32_t n,
                                                                 uint32_t mask, uint32_t* __restrict__ pos) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= k) return;
  uint32_t p[8], bad = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint4 t = names[4u * j + q];
    p[2 * q] = (unhex4(t.x, bad) << 16) | unhex4(t.y, bad);
    p[2 * q + 1] = (unhex4(t.z, bad) << 16) | unhex4(t.w, bad);
  }
  uint32_t found = POW_POOL_NONE;
  if (!bad) {
    const uint4 a = make_uint4(p[0], p[1], p[2], p[3]), b = make_uint4(p[4], p[5], p[6], p[7]);
    uint32_t slot = b.w & mask;
    for (uint32_t probe = 0; probe <= mask; ++probe) {
      const uint32_t held = table[slot];
      if (held >= n) break;
      if (same_digest(dig, held, a, b)) {
        found = held;
        break;
      }
      slot = (slot + 1u) & mask;
    }
  }
  pos[j] = found;
}

// D.n: the pool's blocks after the add; base: before it.  Each launches over
// the new blocks only, but the join, which scans the old ones too.
hipError_t pow_launch_pool_live_insert(hipStream_t stream, const PowPoolDev& D, uint32_t base) {
  hipLaunchKernelGGL(pow_pool_live_insert_kernel, dim3((D.n - base + 255u) / 256u), dim3(256), 0, stream, D.status,
                     (const uint4*)D.dig, D.table, base, D.n, D.slots - 1u, D.ctl);
  return hipGetLastError();
}

// The ranking's first state goes into the buffers 0, as K10c's.
hipError_t pow_launch_pool_live_join(hipStream_t stream, const PowPoolDev& D, uint32_t base) {
  hipLaunchKernelGGL(pow_pool_live_join_kernel, dim3((D.n + 255u) / 256u), dim3(256), 0, stream, D.status, D.kind,
                     (const uint4*)D.dig, (const uint4*)D.prev, D.index, D.table, base, D.n, D.slots - 1u, D.parent,
                     D.next[0], D.depth[0], D.bad[0], (PowPoolLiveCtl*)D.ctl);
  return hipGetLastError();
}

// Reads the buffers `from` and writes the others.
hipError_t pow_launch_pool_live_round(hipStream_t stream, const PowPoolDev& D, uint32_t base, uint32_t from) {
  const uint32_t a = from & 1u, b = a ^ 1u;
  hipLaunchKernelGGL(pow_pool_live_round_kernel, dim3((D.n - base + 255u) / 256u), dim3(256), 0, stream, base, D.n,
                     D.next[a], D.depth[a], D.bad[a], D.next[b], D.depth[b], D.bad[b]);
  return hipGetLastError();
}

// which: the buffers the last round wrote; fin: the pool's final buffers.
hipError_t pow_launch_pool_live_finish(hipStream_t stream, const PowPoolDev& D, uint32_t base, uint32_t which,
                                       uint32_t fin) {
  hipLaunchKernelGGL(pow_pool_live_finish_kernel, dim3((D.n - base + 255u) / 256u), dim3(256), 0, stream, base, D.n,
                     D.next[which], D.depth[which], D.bad[which], D.depth[fin], D.bad[fin], D.status, D.index, D.ctl);
  return hipGetLastError();
}

hipError_t pow_launch_pool_live_strip(hipStream_t stream, const PowPoolDev& D) {
  const uint32_t words = (D.n + 3u) / 4u;
  hipLaunchKernelGGL(pow_pool_live_strip_kernel, dim3((words + 255u) / 256u), dim3(256), 0, stream,
                     (uint32_t*)D.status, words);
  return hipGetLastError();
}

hipError_t pow_launch_pool_live_find(hipStream_t stream, const PowPoolDev& D, const uint32_t* names, uint32_t k,
                                     uint32_t* pos) {
  hipLaunchKernelGGL(pow_pool_live_find_kernel, dim3((k + 255u) / 256u), dim3(256), 0, stream, (const uint4*)names, k,
                     (const uint4*)D.dig, D.table, D.n, D.slots - 1u, pos);
  return hipGetLastError();
}
