// What the fused mining kernels K4 (pow_chain.hip), K5 (pow_batch.hip) and K6
// (pow_race.hip) share: a workgroup's search for the lowest solving key of one
// template, how it leaves, and what the last one out does with the winner.
// Each kernel is one translation unit that includes this header; a kernel
// keeps how blockIdx.x maps to (template or rival, part), where word 0 of the
// message comes from, which control words it uses, and what its last
// workgroup writes.  K8 (pow_rand.hip) walks the reference's rand() nonces with
// a loop of its own and shares the rest: expand, trial_of, leave and winner.
//
// The message. A template is a 552-byte struct Block in LDS as 138 dwords;
// its padded message is 80 words in 5 chunks.  Message bytes 4..269 are the
// struct's nonce and previous_block_hash, 266 bytes that start 2 bytes past a
// dword of the struct, so they are byte-swapped dwords of it.  The hash field
// is read from dwords base + 3 .. base + 67: base = 5 for a struct's own
// previous_block_hash (K5), base = 69 for the parent's block_hash, all 256
// bytes of it (trap T5), which the template refresh makes the next block's
// previous_block_hash (K4, K6):
//   word 0      = the low bytes of index, owner, difficulty, created_at: the caller's
//   words 1, 2  = nonce[0..7], word 3 = nonce[8], NUL, hash[0], hash[1]
//                 (the nonce bytes zero here: a trial ORs its own in)
//   word k, 4 <= k <= 66 = byte-swapped dword base + k
//   word 67     = hash[254], hash[255], the 0x80 pad byte, zero
//   words 68..78 = 0, word 79 = 2160.
// Chunks 1-4 do not hold the nonce: four lanes expand their message schedules
// once per workgroup into LDS with K folded in (what pow_build_consts does on
// the host for K1), so a trial is one generic compression (chunk 0,
// sha256_dev.h's compress, as K3) and 4 x 64 rounds that read K + W.
//
// The walk.  A template's search has `nparts` workgroups; lane g of its
// G = 256 x nparts lanes tests the relative counters g, g + G, g + 2G, ... in
// ascending order.  Every trial has a key, ascending in the counter (K4, K5: the
// counter; K6: counter << 8 | rival), and all lanes that compete share one
// word, the lowest solving key published so far (an atomic min in device
// memory).  A lane stops at its first hit, at the end of the window, or once
// its next key lies above that word.  The word only ever holds the key of a
// trial that solved, so a lane never skips a key below the answer: every key
// below the answer is tested, whatever the grid is, and the word ends as the
// lowest solving key of the window.  With EARLY the workgroup reads the word
// before its first trial too, and one whose lowest key already lies above it
// expands nothing and tests nothing: a grid may be many times what the chip
// holds, so a workgroup may start long after the answer is known (K5, K6).
// K4's grid never exceeds the chip, and it does without that read.
//
// Nobody waits.  No workgroup waits for another (with grids beyond residency
// such a wait would hang).  A workgroup stores its lowest hit with its digest
// in its slot (one writer: a key belongs to one lane), fences, and counts
// itself out with one atomic add on the exit word that also carries its trial
// count.  The one that counts n - 1 others is the last to leave: every slot
// was written and fenced before its workgroup's add, so after a fence of its
// own the last one reads them all, finds the slot of the lowest key, and
// writes the result.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pow_ctx.h"
#include "sha256_dev.h"

namespace powwalk {

using namespace powdev;

constexpr uint32_t WG = 256;
constexpr uint32_t BLK_DW = sizeof(pow_block) / 4;  // 138
static_assert(sizeof(pow_block) == 552 && offsetof(pow_block, created_at) == 16 && offsetof(pow_block, nonce) == 24 &&
                  offsetof(pow_block, previous_block_hash) == 34 && offsetof(pow_block, block_hash) == 290,
              "the kernels' offsets are those of the reference's struct Block");
constexpr uint32_t EXIT_BITS = 16;  // of the exit word: the workgroups that left; their trials above
static_assert(POW_WALK_MAX_WG == 1u << EXIT_BITS, "the exit word counts POW_WALK_MAX_WG - 1 others");

// block.cpp:61-72's alphabet.
__device__ __forceinline__ uint32_t digit_char(uint32_t d) {
  return d < 26u ? 'a' + d : d < 52u ? 'A' + d - 26u : '0' + d - 52u;
}

// The nine nonce characters of ctr_start + rel: rel's six base-62 digits
// (rel < 2^32 < 62^6) added to ctr_start's nine with carry, all in 32 bits.
__device__ __forceinline__ void nonce_chars(const uint32_t (&base_digit)[9], uint32_t rel, uint32_t c[9]) {
  uint32_t carry = 0;
#pragma unroll
  for (int i = 8; i >= 0; --i) {
    uint32_t d = base_digit[i] + carry;
    if (i >= 3) {
      d += rel % 62u;
      rel /= 62u;
    }
    carry = d >= 62u ? 1u : 0u;
    c[i] = digit_char(d - 62u * carry);
  }
}

// Word k (0..79) of the padded message, nonce bytes zero, from the struct `blk` in LDS.
__device__ __forceinline__ uint32_t message_word(const uint32_t* blk, uint32_t base, uint32_t w0, uint32_t k) {
  if (k == 0u) return w0;
  if (k == 3u) return __builtin_bswap32(blk[base + 3u]) & 0xFFFFu;
  if (k >= 4u && k <= 66u) return __builtin_bswap32(blk[base + k]);
  if (k == 67u) return (__builtin_bswap32(blk[base + 67u]) & 0xFFFF0000u) | 0x8000u;
  if (k == 79u) return POW_MSG_BYTES * 8u;
  return 0u;
}

template <class T>
__device__ __forceinline__ T load_agent(const T* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A workgroup's LDS for the walk and for leaving.
template <bool EARLY>
struct SeenWord {
  unsigned long long seen;  // the lowest key as this workgroup found it
};
template <>
struct SeenWord<false> {};
template <bool EARLY>
struct WalkLds : SeenWord<EARLY> {
  uint32_t msg0[16];   // chunk 0 of the message, nonce words zero
  uint32_t kw[4][64];  // chunks 1-4: K[i] + W[i]
  unsigned long long wg_min;
  unsigned long long wg_trials;
  unsigned long long left;  // what the exit word held before this workgroup
  uint32_t win_digest[8];   // the last workgroup only
};

// What a lane brings out of the walk.
struct Hit {
  unsigned long long key;  // the lane's solving key; ~0 = none
  uint32_t digest[8];
  uint32_t trials;
};

// msg0 and kw from the struct in LDS.
__device__ __forceinline__ void expand(uint32_t (&msg0)[16], uint32_t (&kw)[4][64], const uint32_t* blk, uint32_t base,
                                       uint32_t w0) {
  const uint32_t tid = threadIdx.x;
  if (tid < 16u) msg0[tid] = message_word(blk, base, w0, tid);
  // Every lane expands one of chunks 1-4 (no divergence); lanes 0-3 keep theirs.
  const uint32_t c = tid & 3u;
  uint32_t w[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) w[k] = message_word(blk, base, w0, 16u * (c + 1u) + k);
#pragma unroll
  for (int i = 0; i < 64; ++i) {
    if (i >= 16) w[i & 15] = ssig1(w[(i + 14) & 15]) + w[(i + 9) & 15] + ssig0(w[(i + 1) & 15]) + w[i & 15];
    if (tid < 4u) kw[c][i] = K[i] + w[i & 15];
  }
}

// The digest of the message with the nine nonce characters that chars(c) gives.
template <class Chars>
__device__ __forceinline__ void trial_of(Chars chars, const uint32_t (&msg0)[16], const uint32_t (&kw)[4][64],
                                         uint32_t h[8]) {
  uint32_t c[9];
  chars(c);
  uint32_t w[16];
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
}

// The digest of the message with the nonce of ctr_start + rel.
__device__ __forceinline__ void trial(const uint32_t (&base_digit)[9], uint32_t rel, const uint32_t (&msg0)[16],
                                      const uint32_t (&kw)[4][64], uint32_t h[8]) {
  trial_of([&](uint32_t (&c)[9]) { nonce_chars(base_digit, rel, c); }, msg0, kw, h);
}

// This workgroup's share, part `part` of `nparts`, of the search over the
// template in `blk`, which the caller has stored in LDS and not yet
// synchronised.  key(rel) is the trial's key; word0() is word 0 of the
// message, evaluated by workgroups that search; min_key is the word the
// competing lanes share.  Ends behind a barrier, with the workgroup's lowest
// hit in sh.wg_min and its trials in sh.wg_trials.
template <bool EARLY, class Key, class Word0>
__device__ __forceinline__ Hit walk(WalkLds<EARLY>& sh, const PowWalkHead& L, const uint32_t* blk, uint32_t base,
                                    Word0 word0, uint32_t part, uint32_t nparts, unsigned long long* min_key, Key key) {
  const uint32_t tid = threadIdx.x;
  if (tid == 0) {
    if constexpr (EARLY) sh.seen = load_agent(min_key);
    sh.wg_min = ~0ull;
    sh.wg_trials = 0ull;
  }
  __syncthreads();
  unsigned long long seen = ~0ull;  // without the early read nothing counts as published: the first trial needs no look
  if constexpr (EARLY) seen = sh.seen;
  Hit me;
  me.key = ~0ull;
#pragma unroll
  for (int k = 0; k < 8; ++k) me.digest[k] = 0u;
  me.trials = 0;
  // Workgroup-uniform: every key of this workgroup lies above a published hit.
  const bool late = key((uint64_t)part * WG) > seen;
  if (!late) {
    expand(sh.msg0, sh.kw, blk, base, word0());
    __syncthreads();
    const uint64_t stride = (uint64_t)nparts * WG;
    uint64_t rel = (uint64_t)part * WG + tid;
    bool go = rel < L.count && key(rel) <= seen;
    while (go) {
      uint32_t h[8];
      trial(L.base_digit, (uint32_t)rel, sh.msg0, sh.kw, h);
      ++me.trials;
      if (h[0] <= L.thr) {
        me.key = key(rel);
#pragma unroll
        for (int k = 0; k < 8; ++k) me.digest[k] = h[k];
        atomicMin(min_key, me.key);
        break;  // the lane's later counters are higher
      }
      rel += stride;
      go = rel < L.count && key(rel) <= load_agent(min_key);
    }
    if (me.key != ~0ull) atomicMin(&sh.wg_min, me.key);
    if (me.trials) atomicAdd(&sh.wg_trials, (unsigned long long)me.trials);
  }
  __syncthreads();
  return me;
}

struct Exit {
  bool last;                  // this workgroup counted n - 1 others: every other one has left
  unsigned long long trials;  // theirs and this one's
};

// This workgroup's lowest hit into its slot, then out: one of the n workgroups that share the exit word.
template <bool EARLY>
__device__ __forceinline__ Exit leave(WalkLds<EARLY>& sh, const Hit& me, PowChainSlot* slot, unsigned long long* exit_word,
                                      uint32_t n) {
  const uint32_t tid = threadIdx.x;
  const unsigned long long mine = sh.wg_min;
  if (mine == ~0ull ? tid == 0u : me.key == mine) {  // a key belongs to one lane: one writer
    slot->rel = mine;
#pragma unroll
    for (int k = 0; k < 8; ++k) slot->digest[k] = me.digest[k];
    __threadfence();
  }
  __syncthreads();
  if (tid == 0) sh.left = atomicAdd(exit_word, (sh.wg_trials << EXIT_BITS) | 1ull);
  __syncthreads();
  const unsigned long long was = sh.left;
  return Exit{(uint32_t)(was & (POW_WALK_MAX_WG - 1u)) == n - 1u, (was >> EXIT_BITS) + sh.wg_trials};
}

// The last workgroup: the lowest solving key (~0 = none) and, in
// sh.win_digest, its digest from the one slot of the n that holds it.  The
// caller synchronises before it reads sh.win_digest.
template <bool EARLY>
__device__ __forceinline__ unsigned long long winner(WalkLds<EARLY>& sh, const unsigned long long* min_key,
                                                     const PowChainSlot* slot, uint32_t n) {
  __threadfence();
  const unsigned long long best = load_agent(min_key);
  for (uint32_t s = threadIdx.x; s < n; s += WG) {
    const unsigned long long r = load_agent(&slot[s].rel);
    uint32_t d[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = load_agent(&slot[s].digest[k]);
    if (r == best && best != ~0ull) {  // exactly one slot
#pragma unroll
      for (int k = 0; k < 8; ++k) sh.win_digest[k] = d[k];
    }
  }
  return best;
}

// ---- K4 and K6: launches queued behind each other, each sealing a block on its parent ----

// Their LDS, one object so that it packs as tightly as separate arrays did.
template <bool EARLY>
struct SealerLds {
  uint32_t par[BLK_DW];    // the parent
  uint32_t block[BLK_DW];  // the sealed block (the last workgroup only)
  uint32_t nonce[9];       // its nonce characters
  WalkLds<EARLY> walk;
};

// The parent into LDS.  False: an earlier launch of the batch found no
// solution, and this one exits at its first read.
__device__ __forceinline__ bool load_parent(uint32_t (&par)[BLK_DW], const uint32_t* __restrict__ prev,
                                            const PowSealCtl* ctl) {
  const uint32_t tid = threadIdx.x;
  const uint32_t p = tid < BLK_DW ? prev[tid] : 0u;  // in flight together with the stop word
  if (ctl->stop != 0u) return false;                 // written by an earlier launch only
  if (tid < BLK_DW) par[tid] = p;
  return true;
}

// The last workgroup closes the launch's account.  False: no window held a
// solution; the launches queued behind exit at their first read.
__device__ __forceinline__ bool close_launch(PowSealCtl* ctl, unsigned long long trials, unsigned long long best) {
  if (threadIdx.x == 0) {
    ctl->hashes += trials;
    ctl->exits = 0ull;
    if (best == ~0ull) ctl->stop = 1u;
  }
  return best != ~0ull;
}

// The success tail of node.cpp:311-318 by the last workgroup: the 552 bytes
// of the block on sh.par, with the digest winner() left, into dst (the parent
// copied whole, padding included; bytes 65..255 of block_hash stay the
// parent's, node.cpp:318), and the control words reset for the next launch.
template <bool EARLY>
__device__ __forceinline__ void seal(SealerLds<EARLY>& sh, const uint32_t (&base_digit)[9], uint32_t win_rel,
                                     uint32_t owner, uint32_t diff, uint64_t created_at, uint32_t* __restrict__ dst,
                                     PowSealCtl* ctl) {
  const uint32_t tid = threadIdx.x;
  if (tid == 0) {
    uint32_t c[9];
    nonce_chars(base_digit, win_rel, c);
#pragma unroll
    for (int k = 0; k < 9; ++k) sh.nonce[k] = c[k];
  }
  __syncthreads();
  const uint8_t* const pb = (const uint8_t*)sh.par;
  uint8_t* const sb = (uint8_t*)sh.block;
  const uint32_t index = sh.par[0] + 1u;
  for (uint32_t i = tid; i < (uint32_t)sizeof(pow_block); i += WG) {
    uint32_t v = pb[i];  // the parent's byte: padding, and block_hash[65..255]
    if (i < 4u) v = index >> (8u * i);
    else if (i < 8u) v = owner >> (8u * (i - 4u));
    else if (i < 12u) v = diff >> (8u * (i - 8u));
    else if (i >= 16u && i < 24u) v = (uint32_t)(created_at >> (8u * (i - 16u)));
    else if (i >= 24u && i < 33u) v = sh.nonce[i - 24u];
    else if (i == 33u) v = 0u;
    else if (i >= 34u && i < 290u) v = pb[i + 256u];  // previous_block_hash = the parent's block_hash
    else if (i >= 290u && i < 354u) {
      const uint32_t j = i - 290u;
      const uint32_t nib = (sh.walk.win_digest[j >> 3] >> (28u - 4u * (j & 7u))) & 15u;
      v = nib < 10u ? '0' + nib : 'a' + nib - 10u;
    } else if (i == 354u) v = 0u;
    sb[i] = (uint8_t)v;
  }
  __syncthreads();
  if (tid < BLK_DW) dst[tid] = sh.block[tid];
  if (tid == 0) {
    ctl->min_key = ~0ull;
    ctl->n_done += 1u;
  }
}

}  // namespace powwalk
