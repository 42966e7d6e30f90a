// K5  pow_batch_kernel — one tile of pow_mine_batch per launch: many
// independent templates, each with its own lowest-counter search (K4's), over
// the raw 552-byte structs as K3 reads them.
//
// The grid is flat and one-dimensional (gridDim.y stops at 65,535): workgroup
// w serves template w / nwg_t as part w % nwg_t of that template's nwg_t
// workgroups.  A workgroup belongs to one template.
//
// The workgroup copies its template's 138 dwords into LDS and derives the 80
// message words from the struct itself (K3's layout fact: message bytes 4..269
// are struct bytes 24..289, a shift of 20 bytes):
//   word 0      = the low bytes of index, owner, difficulty, created_at
//   words 1, 2  = nonce[0..7], word 3 = nonce[8], NUL, prev[0], prev[1]
//                 (the nonce bytes zero here: a trial ORs its own in)
//   word k, 4 <= k <= 66 = byte-swapped struct dword k + 5
//   word 67     = prev[254], prev[255], the 0x80 pad byte, zero
//   words 68..78 = 0, word 79 = 2160.
// Chunks 1-4 do not hold the nonce: four lanes expand their message schedules
// once per workgroup into LDS with K folded in, so a trial is one generic
// compression (chunk 0) and 4 x 64 rounds that read K + W, as K4.
//
// The search, per template: lane g of the template's G = 256 x nwg_t lanes
// tests the relative counters g, g + G, g + 2G, ... in ascending order and
// stops at its first hit, at the end of the window, or once its next counter
// lies above the lowest hit any lane of the template has published (an atomic
// min on the template's min_rel).  A grid may be many times what the chip
// holds, so a workgroup may start long after its template is solved: it reads
// min_rel before its first trial too, and a workgroup whose lowest counter
// already lies above it expands nothing and tests nothing.  A counter below
// the answer is always tested, whatever G is.
//
// No workgroup waits for another (with grids beyond residency such a wait
// would hang).  A workgroup stores its lowest hit with its digest in its slot,
// fences, and counts itself out on its template's exit word (one atomic add
// that also carries its trial count); the one that counts nwg_t - 1 others is
// the template's last to leave and writes the template's result record from
// the slots.  The host resets the control words per tile and seals the blocks.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pow_ctx.h"
#include "sha256_dev.h"

using namespace powdev;

namespace {

constexpr uint32_t WG = 256;
constexpr uint32_t BLK_DW = sizeof(pow_block) / 4;  // 138
static_assert(sizeof(pow_block) == 552 && offsetof(pow_block, created_at) == 16 && offsetof(pow_block, nonce) == 24 &&
                  offsetof(pow_block, previous_block_hash) == 34 && offsetof(pow_block, block_hash) == 290,
              "the kernel's offsets are those of the reference's struct Block");
static_assert(sizeof(PowBatchRec) == 48 && sizeof(PowBatchCtl) == 16, "the host reads the records as they are");

// block.cpp:61-72's alphabet.
__device__ __forceinline__ uint32_t digit_char(uint32_t d) {
  return d < 26u ? 'a' + d : d < 52u ? 'A' + d - 26u : '0' + d - 52u;
}

// The nine nonce characters of ctr_start + rel: rel's six base-62 digits
// (rel < 2^32 < 62^6) added to ctr_start's nine with carry, all in 32 bits.
__device__ __forceinline__ void nonce_chars(const PowBatchLaunch& L, uint32_t rel, uint32_t c[9]) {
  uint32_t carry = 0;
#pragma unroll
  for (int i = 8; i >= 0; --i) {
    uint32_t d = L.base_digit[i] + carry;
    if (i >= 3) {
      d += rel % 62u;
      rel /= 62u;
    }
    carry = d >= 62u ? 1u : 0u;
    c[i] = digit_char(d - 62u * carry);
  }
}

// Word k (0..79) of the template's padded message, nonce bytes zero, from the struct in LDS.
__device__ __forceinline__ uint32_t message_word(const uint32_t* t, uint32_t k) {
  if (k == 0u) return (t[0] << 24) | ((t[1] & 0xFFu) << 16) | ((t[2] & 0xFFu) << 8) | (t[4] & 0xFFu);
  if (k == 1u || k == 2u) return 0u;
  if (k == 3u) return __builtin_bswap32(t[8]) & 0xFFFFu;
  if (k <= 66u) return __builtin_bswap32(t[k + 5u]);
  if (k == 67u) return (__builtin_bswap32(t[72]) & 0xFFFF0000u) | 0x8000u;
  if (k == 79u) return POW_MSG_BYTES * 8u;
  return 0u;
}

template <class T>
__device__ __forceinline__ T load_agent(const T* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

__global__ __launch_bounds__(256) void pow_batch_kernel(const PowBatchLaunch L, const uint32_t* __restrict__ tmpls,
                                                        PowBatchCtl* ctls, PowChainSlot* slots,
                                                        PowBatchRec* __restrict__ recs) {
  __shared__ uint32_t tm[BLK_DW];  // the template
  __shared__ uint32_t msg0[16];    // chunk 0 of its message, nonce words zero
  __shared__ uint32_t kw[4][64];   // chunks 1-4: K[i] + W[i]
  __shared__ unsigned long long wg_min;
  __shared__ unsigned long long wg_trials;
  __shared__ unsigned long long seen;  // the template's minimum as this workgroup found it
  __shared__ unsigned long long left;  // what the exit count held before this workgroup
  __shared__ uint32_t win_digest[8];
  const uint32_t tid = threadIdx.x;
  const uint32_t t = blockIdx.x / L.nwg_t;
  const uint32_t part = blockIdx.x - t * L.nwg_t;
  PowBatchCtl* const ctl = ctls + t;
  if (tid < BLK_DW) tm[tid] = tmpls[(size_t)t * BLK_DW + tid];
  if (tid == 0) {
    seen = load_agent(&ctl->min_rel);
    wg_min = ~0ull;
    wg_trials = 0ull;
  }
  if (tid < 8u) win_digest[tid] = 0u;
  __syncthreads();
  // Workgroup-uniform: every counter of this workgroup lies above a published hit.
  const bool late = (uint64_t)part * WG > seen;

  uint64_t hit = ~0ull;
  uint32_t dg[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) dg[k] = 0u;
  uint32_t trials = 0;
  if (!late) {
    if (tid < 16u) msg0[tid] = message_word(tm, tid);
    {
      // Every lane expands one of chunks 1-4 (no divergence); lanes 0-3 keep theirs.
      const uint32_t c = tid & 3u;
      uint32_t w[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) w[k] = message_word(tm, 16u * (c + 1u) + k);
#pragma unroll
      for (int i = 0; i < 64; ++i) {
        if (i >= 16) w[i & 15] = ssig1(w[(i + 14) & 15]) + w[(i + 9) & 15] + ssig0(w[(i + 1) & 15]) + w[i & 15];
        if (tid < 4u) kw[c][i] = K[i] + w[i & 15];
      }
    }
    __syncthreads();

    // ---- the search ----
    const uint64_t stride = (uint64_t)L.nwg_t * WG;
    uint64_t rel = (uint64_t)part * WG + tid;
    bool go = rel < L.count && rel <= seen;
    while (go) {
      uint32_t c[9];
      nonce_chars(L, (uint32_t)rel, c);
      uint32_t h[8], w[16];
#pragma unroll
      for (int k = 0; k < 8; ++k) h[k] = IV[k];
#pragma unroll
      for (int k = 0; k < 16; ++k) w[k] = msg0[k];
      w[1] = (c[0] << 24) | (c[1] << 16) | (c[2] << 8) | c[3];
      w[2] = (c[4] << 24) | (c[5] << 16) | (c[6] << 8) | c[7];
      w[3] |= c[8] << 24;
      compress(h, w);
#pragma unroll 1
      for (uint32_t c4 = 0; c4 < 4u; ++c4) {
        St s{h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7]};
#pragma unroll
        for (int i = 0; i < 64; ++i) round_k_w(s, kw[c4][i], 0u);
        h[0] += s.a; h[1] += s.b; h[2] += s.c; h[3] += s.d;
        h[4] += s.e; h[5] += s.f; h[6] += s.g; h[7] += s.h;
      }
      ++trials;
      if (h[0] <= L.thr) {
        hit = rel;
#pragma unroll
        for (int k = 0; k < 8; ++k) dg[k] = h[k];
        atomicMin(&ctl->min_rel, (unsigned long long)rel);
        break;  // the lane's later counters are higher
      }
      rel += stride;
      go = rel < L.count && rel <= load_agent(&ctl->min_rel);
    }
    if (hit != ~0ull) atomicMin(&wg_min, (unsigned long long)hit);
    if (trials) atomicAdd(&wg_trials, (unsigned long long)trials);
  }
  __syncthreads();

  // ---- this workgroup's lowest hit into its slot, then out ----
  const unsigned long long mine = wg_min;
  PowChainSlot* const tslots = slots + (size_t)t * L.nwg_t;
  PowChainSlot* const slot = tslots + part;
  if (mine == ~0ull ? tid == 0u : hit == mine) {  // a counter belongs to one lane: one writer
    slot->rel = mine;
#pragma unroll
    for (int k = 0; k < 8; ++k) slot->digest[k] = dg[k];
    __threadfence();
  }
  __syncthreads();
  if (tid == 0) {
    // One atomic: the template's workgroups that left (low 24 bits; nwg_t <= 2^24)
    // and their trials above them (at most 2^32 + one per lane).
    left = atomicAdd(&ctl->exits, (wg_trials << 24) | 1ull);
  }
  __syncthreads();
  if ((uint32_t)(left & 0xFFFFFFull) != L.nwg_t - 1u) return;

  // ---- the template's last workgroup out writes its record; every other one has left ----
  __threadfence();
  const unsigned long long best = load_agent(&ctl->min_rel);
  for (uint32_t s = tid; s < L.nwg_t; s += WG) {
    const unsigned long long r = load_agent(&tslots[s].rel);
    uint32_t d[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = load_agent(&tslots[s].digest[k]);
    if (r == best && best != ~0ull) {  // exactly one slot
#pragma unroll
      for (int k = 0; k < 8; ++k) win_digest[k] = d[k];
    }
  }
  __syncthreads();
  if (tid == 0) {
    PowBatchRec* const rec = recs + t;
    rec->rel = best;
#pragma unroll
    for (int k = 0; k < 8; ++k) rec->digest[k] = win_digest[k];
    rec->trials = (left >> 24) + wg_trials;
  }
}

// n_tmpl x L.nwg_t workgroups: the caller keeps the product at POW_BATCH_MAX_WG or below.
hipError_t pow_launch_batch(hipStream_t stream, const PowBatchLaunch& L, uint32_t n_tmpl, const uint32_t* tmpls,
                            PowBatchCtl* ctl, PowChainSlot* slots, PowBatchRec* rec) {
  if (n_tmpl == 0) return hipSuccess;
  if (L.nwg_t == 0 || (uint64_t)n_tmpl * L.nwg_t > POW_BATCH_MAX_WG || n_tmpl > POW_BATCH_MAX_TILE)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(pow_batch_kernel, dim3(n_tmpl * L.nwg_t), dim3(WG), 0, stream, L, tmpls, ctl, slots, rec);
  return hipGetLastError();
}
