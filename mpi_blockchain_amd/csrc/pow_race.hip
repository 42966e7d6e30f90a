// K6  pow_race_kernel — one height of pow_mine_race per launch: N rival miners
// (node.cpp:292-302: every rank refreshes its own template on the same tip),
// each with K4's template refresh and lowest-counter search, under ONE minimum
// shared by all of them, and K4's success tail for the winner alone.
//
// A launch reads the block before it (`prev`: the caller's parent for the
// first launch of a batch, else the block the launch before it sealed) and
// writes the winner's sealed block (`dst`) and the height's record.  The
// launches of a batch are queued on one stream, so a launch sees what its
// predecessor wrote (kernel boundaries order them); inside a launch `prev` is
// only read and `dst` only written.
//
// The grid is flat: workgroup w serves rival w % R as part w / R of that
// rival's nwg_r workgroups, so the workgroups that start first hold every
// rival's lowest counters.  A workgroup belongs to one rival: it reads the
// parent and its rival's owner and created_at (device arrays that went up once
// per batch) and derives the template's 80 message words as K4 does.
// previous_block_hash of the template is the parent's block_hash, all 256
// bytes (trap T5), which starts at struct byte 290:
//   word 0      = the low bytes of index + 1, owner, difficulty, created_at
//   words 1, 2  = nonce[0..7], word 3 = nonce[8], NUL, hash[0], hash[1]
//   word k, 4 <= k <= 66 = byte-swapped struct dword 69 + k (hash[4k-14..])
//   word 67     = hash[254], hash[255], the 0x80 pad byte, zero
//   words 68..78 = 0, word 79 = 2160.
// Only word 0 differs between two rivals, and only in two bytes: rivals whose
// owners and created_at agree in their low bytes have identical digests.
// Chunks 1-4 do not hold the nonce: four lanes expand their message schedules
// once per workgroup into LDS with K folded in, so a trial is one generic
// compression (chunk 0) and 4 x 64 rounds that read K + W, as K4.
//
// The race: a pair (relative counter rel, rival r) has the key rel << 8 | r,
// and the winner of the height is the solving pair with the lowest key: the
// lowest counter, ties to the lowest position.  Lane g of rival r's G = 256 x
// nwg_r lanes tests rel = g, g + G, g + 2G, ... in ascending order and stops at
// its first hit, at the end of the window, or once its next key lies above the
// lowest key any lane of any rival has published (an atomic min on one word per
// launch).  It reads that word before its first trial too, and a workgroup
// whose lowest key already lies above it expands nothing and tests nothing.  A
// pair below the answer is therefore always tested, whatever the grid is, and
// a height costs about the trials of one solo block, not R times that.
//
// No workgroup waits for another.  A workgroup stores its lowest hit with its
// digest in its slot, fences, and counts itself out (one atomic add that also
// carries its trial count); the one that counts the grid - 1 others is the last
// to leave and seals the block: it finds the slot of the lowest key, writes the
// 552 bytes with the winner's owner and created_at (the parent copied whole,
// padding included; bytes 65..255 of block_hash stay the parent's,
// node.cpp:318), writes the record and resets the launch's words for the next
// launch.  A height nobody solves raises `stop` instead: the launches queued
// behind exit at their first read.
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
static_assert(POW_RACE_MAX_RIVALS == 256, "a key carries the rival in its low 8 bits");
static_assert(sizeof(PowRaceRec) == 16 && sizeof(PowRaceCtl) == 32, "the host reads the records as they are");

// block.cpp:61-72's alphabet.
__device__ __forceinline__ uint32_t digit_char(uint32_t d) {
  return d < 26u ? 'a' + d : d < 52u ? 'A' + d - 26u : '0' + d - 52u;
}

// The nine nonce characters of ctr_start + rel: rel's six base-62 digits
// (rel < 2^32 < 62^6) added to ctr_start's nine with carry, all in 32 bits.
__device__ __forceinline__ void nonce_chars(const PowRaceLaunch& L, uint32_t rel, uint32_t c[9]) {
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

// Word k (0..79) of a rival's padded message, nonce bytes zero, from the parent in LDS.
__device__ __forceinline__ uint32_t message_word(const uint32_t* par, uint32_t diff, uint32_t owner, uint32_t created_lo,
                                                 uint32_t k) {
  if (k == 0u) return ((par[0] + 1u) << 24) | ((owner & 0xFFu) << 16) | ((diff & 0xFFu) << 8) | (created_lo & 0xFFu);
  if (k == 3u) return __builtin_bswap32(par[72]) & 0xFFFFu;
  if (k >= 4u && k <= 66u) return __builtin_bswap32(par[69u + k]);
  if (k == 67u) return (__builtin_bswap32(par[136]) & 0xFFFF0000u) | 0x8000u;
  if (k == 79u) return POW_MSG_BYTES * 8u;
  return 0u;
}

template <class T>
__device__ __forceinline__ T load_agent(const T* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace

__global__ __launch_bounds__(256) void pow_race_kernel(const PowRaceLaunch L, const uint32_t* __restrict__ prev,
                                                       uint32_t* __restrict__ dst, const PowRaceIn* __restrict__ in,
                                                       PowRaceCtl* ctl, PowChainSlot* slots,
                                                       PowRaceRec* __restrict__ recs) {
  __shared__ uint32_t par[BLK_DW];   // the parent
  __shared__ uint32_t msg0[16];      // chunk 0 of the rival's message, nonce words zero
  __shared__ uint32_t kw[4][64];     // chunks 1-4: K[i] + W[i]
  __shared__ uint32_t seal[BLK_DW];  // the sealed block (the last workgroup only)
  __shared__ unsigned long long wg_min;
  __shared__ unsigned long long wg_trials;
  __shared__ unsigned long long seen;  // the launch's minimum as this workgroup found it
  __shared__ unsigned long long left;  // what the exit count held before this workgroup
  __shared__ uint32_t win_digest[8];
  __shared__ uint32_t win_nonce[9];
  const uint32_t tid = threadIdx.x;
  const uint32_t part = blockIdx.x / L.n_rivals;
  const uint32_t r = blockIdx.x - part * L.n_rivals;
  const uint32_t nwg = L.nwg_r * L.n_rivals;
  {
    const uint32_t p = tid < BLK_DW ? prev[tid] : 0u;  // in flight together with the stop word
    if (ctl->stop != 0u) return;                       // written by an earlier launch only
    if (tid < BLK_DW) par[tid] = p;
    if (tid == 0) {
      seen = load_agent(&ctl->min_key);
      wg_min = ~0ull;
      wg_trials = 0ull;
    }
  }
  __syncthreads();
  // Workgroup-uniform: every key of this workgroup lies above a published hit.
  const bool late = ((((uint64_t)part * WG) << 8) | r) > seen;

  uint64_t hit = ~0ull;  // this lane's solving key
  uint32_t dg[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) dg[k] = 0u;
  uint32_t trials = 0;
  if (!late) {
    const uint32_t owner = in->owner[r];
    const uint32_t created_lo = (uint32_t)in->created_at[(size_t)L.height * L.n_rivals + r];
    if (tid < 16u) msg0[tid] = message_word(par, L.diff, owner, created_lo, tid);
    {
      // Every lane expands one of chunks 1-4 (no divergence); lanes 0-3 keep theirs.
      const uint32_t c = tid & 3u;
      uint32_t w[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) w[k] = message_word(par, L.diff, owner, created_lo, 16u * (c + 1u) + k);
#pragma unroll
      for (int i = 0; i < 64; ++i) {
        if (i >= 16) w[i & 15] = ssig1(w[(i + 14) & 15]) + w[(i + 9) & 15] + ssig0(w[(i + 1) & 15]) + w[i & 15];
        if (tid < 4u) kw[c][i] = K[i] + w[i & 15];
      }
    }
    __syncthreads();

    // ---- the search ----
    const uint64_t stride = (uint64_t)L.nwg_r * WG;
    uint64_t rel = (uint64_t)part * WG + tid;
    bool go = rel < L.count && ((rel << 8) | r) <= seen;
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
        hit = (rel << 8) | r;
#pragma unroll
        for (int k = 0; k < 8; ++k) dg[k] = h[k];
        atomicMin(&ctl->min_key, (unsigned long long)hit);
        break;  // the lane's later counters are higher
      }
      rel += stride;
      go = rel < L.count && ((rel << 8) | r) <= load_agent(&ctl->min_key);
    }
    if (hit != ~0ull) atomicMin(&wg_min, (unsigned long long)hit);
    if (trials) atomicAdd(&wg_trials, (unsigned long long)trials);
  }
  __syncthreads();

  // ---- this workgroup's lowest hit into its slot, then out ----
  const unsigned long long mine = wg_min;
  PowChainSlot* const slot = slots + blockIdx.x;
  if (mine == ~0ull ? tid == 0u : hit == mine) {  // a key belongs to one lane: one writer
    slot->rel = mine;
#pragma unroll
    for (int k = 0; k < 8; ++k) slot->digest[k] = dg[k];
    __threadfence();
  }
  __syncthreads();
  if (tid == 0) {
    // One atomic: the workgroups that left (low 16 bits; the grid stays below
    // 2^16) and the launch's trials above them (at most 2^40 + one per lane).
    left = atomicAdd(&ctl->exits, (wg_trials << 16) | 1ull);
  }
  __syncthreads();
  if ((uint32_t)(left & 0xFFFFull) != nwg - 1u) return;

  // ---- the last workgroup out seals the block; every other one has left ----
  __threadfence();
  const unsigned long long best = load_agent(&ctl->min_key);
  for (uint32_t s = tid; s < nwg; s += WG) {
    const unsigned long long key = load_agent(&slots[s].rel);
    uint32_t d[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = load_agent(&slots[s].digest[k]);
    if (key == best && best != ~0ull) {  // exactly one slot
#pragma unroll
      for (int k = 0; k < 8; ++k) win_digest[k] = d[k];
    }
  }
  if (tid == 0) {
    ctl->hashes += (left >> 16) + wg_trials;
    ctl->exits = 0ull;
    if (best == ~0ull) ctl->stop = 1u;
  }
  if (best == ~0ull) return;
  const uint32_t winner = (uint32_t)(best & 0xFFull);
  const uint32_t best_rel = (uint32_t)(best >> 8);
  const uint32_t win_owner = in->owner[winner];
  const uint64_t win_created = in->created_at[(size_t)L.height * L.n_rivals + winner];
  if (tid == 0) {
    uint32_t c[9];
    nonce_chars(L, best_rel, c);
#pragma unroll
    for (int k = 0; k < 9; ++k) win_nonce[k] = c[k];
  }
  __syncthreads();
  const uint8_t* const pb = (const uint8_t*)par;
  uint8_t* const sb = (uint8_t*)seal;
  const uint32_t index = par[0] + 1u;
  for (uint32_t i = tid; i < (uint32_t)sizeof(pow_block); i += WG) {
    uint32_t v = pb[i];  // the parent's byte: padding, and block_hash[65..255]
    if (i < 4u) v = index >> (8u * i);
    else if (i < 8u) v = win_owner >> (8u * (i - 4u));
    else if (i < 12u) v = L.diff >> (8u * (i - 8u));
    else if (i >= 16u && i < 24u) v = (uint32_t)(win_created >> (8u * (i - 16u)));
    else if (i >= 24u && i < 33u) v = win_nonce[i - 24u];
    else if (i == 33u) v = 0u;
    else if (i >= 34u && i < 290u) v = pb[i + 256u];  // previous_block_hash = the parent's block_hash
    else if (i >= 290u && i < 354u) {
      const uint32_t j = i - 290u;
      const uint32_t nib = (win_digest[j >> 3] >> (28u - 4u * (j & 7u))) & 15u;
      v = nib < 10u ? '0' + nib : 'a' + nib - 10u;
    } else if (i == 354u) v = 0u;
    sb[i] = (uint8_t)v;
  }
  __syncthreads();
  if (tid < BLK_DW) dst[tid] = seal[tid];
  if (tid == 0) {
    PowRaceRec* const rec = recs + L.height;
    rec->rel = best_rel;
    rec->winner = winner;
    rec->pad = 0u;
    ctl->min_key = ~0ull;
    ctl->n_done += 1u;
  }
}

// L.n_rivals x L.nwg_r workgroups: the caller keeps the product below POW_RACE_MAX_WG
// and at or below the slots it allocated.
hipError_t pow_launch_race(hipStream_t stream, const PowRaceLaunch& L, const uint32_t* prev, uint32_t* dst,
                           const PowRaceIn* in, PowRaceCtl* ctl, PowChainSlot* slots, PowRaceRec* rec) {
  if (L.n_rivals == 0 || L.n_rivals > POW_RACE_MAX_RIVALS || L.nwg_r == 0 || L.height >= POW_RACE_MAX_BATCH ||
      (uint64_t)L.n_rivals * L.nwg_r >= POW_RACE_MAX_WG)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(pow_race_kernel, dim3(L.n_rivals * L.nwg_r), dim3(WG), 0, stream, L, prev, dst, in, ctl, slots, rec);
  return hipGetLastError();
}
