// What the audit kernels K3 (pow_verify.hip), K7 (pow_verify_batch.hip) and
// K10a (pow_pool.hip) share: the audit of one block from its raw 552-byte
// struct in LDS, in two parts (hash_block: its digest; own_flags: what it shows
// on its own; audit_block: both and the checks against its parent, which K10a
// does not take: a pool's parent is found by name), and the copy of a
// workgroup's tile into LDS.  Each kernel is one translation unit
// that includes this header; a kernel keeps what a lane's block is, whether it
// has a parent in its chain, and where its verdict goes.
//
// Serialisation is free because of a layout fact: the message
// (block_to_str, 270 bytes) is four header bytes followed by nonce[10] and
// previous_block_hash[256], which are struct bytes 24..289.  Message bytes
// 4..269 are therefore struct bytes 24..289, a shift of 20 bytes, a whole
// number of words:
//   message word k, 1 <= k <= 66  = byte-swapped struct dword k + 5
//   word 0   = the low bytes of index, node_owner_number, difficulty and
//              created_at (traps T1/T2/T5: each field is truncated to a char)
//   word 67  = struct bytes 288, 289 (the top half of swapped dword 72), then
//              the 0x80 pad byte and a zero
//   words 68..78 = 0, word 79 = 2160 (270 bytes in bits): 80 words, 5 chunks.
// A lane's block starts at dword 138 * lane of the LDS copy: 138 = 10 mod 64,
// so lanes l and l + 32 share a bank (a 2-way conflict on the per-lane reads).
// The kernels' time is the 320 compression rounds, not their ~100 LDS reads.
//
// The stored hashes sit at struct byte 290 (block_hash) and 34
// (previous_block_hash): both 2 bytes past a dword, so the link check compares
// whole dwords of the two fields (child's dword 8 + j with the parent's dword
// 72 + j), and the hex check shifts the stored text by 16 bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pow_ctx.h"
#include "sha256_dev.h"

namespace powaudit {

using namespace powdev;

constexpr uint32_t BLK_DW = sizeof(pow_block) / 4;  // 138
constexpr uint32_t TILE = 64;                       // blocks per workgroup (one per lane)
constexpr uint32_t TILE_LDS_DW = (TILE + 1) * BLK_DW;  // the tile and its halo block
static_assert(sizeof(pow_block) == 552 && offsetof(pow_block, nonce) == 24 &&
                  offsetof(pow_block, previous_block_hash) == 34 && offsetof(pow_block, block_hash) == 290,
              "the kernels' word offsets are those of the reference's struct Block");

// Four nibbles (each byte of v is 0..15) -> four lowercase hex characters.
__device__ __forceinline__ uint32_t hex4(uint32_t v) {
  const uint32_t above9 = ((v + 0x06060606u) >> 4) & 0x01010101u;
  return v + 0x30303030u + above9 * 39u;
}

// The text of the 16-bit value x as the reference prints it: most significant
// nibble first, i.e. in the lowest byte of the result.
__device__ __forceinline__ uint32_t hex_of16(uint32_t x) {
  return hex4(((x >> 12) & 0xFu) | ((x & 0xF00u)) | ((x & 0xF0u) << 12) | ((x & 0xFu) << 24));
}

// The workgroup's tile into LDS: the min(TILE + 1, n_avail - first) blocks from
// block `first` of `blocks`, the last of them the halo.  64 blocks are 35,328 B,
// a multiple of 16, so every workgroup's source is 16-byte aligned; the copy's
// length (a multiple of 8) may end on a half vector, which goes as two dwords.
// The caller synchronises.
__device__ __forceinline__ void load_tile(uint32_t* lds, const uint32_t* __restrict__ blocks, uint32_t first,
                                          uint32_t n_avail, uint32_t lane) {
  const uint32_t nb = min(TILE + 1u, n_avail - first);
  const uint32_t ndw = nb * BLK_DW, nvec = ndw >> 2;
  const uint32_t* const src = blocks + (size_t)first * BLK_DW;
  const uint4* const src4 = (const uint4*)src;
  uint4* const lds4 = (uint4*)lds;
  for (uint32_t v = lane; v < nvec; v += 64u) lds4[v] = src4[v];
  if (lane < (ndw & 3u)) lds[4u * nvec + lane] = src[4u * nvec + lane];
}

// block_to_hash of the block at b, a raw struct in LDS: its digest into h.
// The one place the audit kernels call the compression.
__device__ __forceinline__ void hash_block(const uint32_t* b, uint32_t h[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) h[k] = IV[k];
#pragma unroll 1
  for (uint32_t c = 0; c < 5; ++c) {
    uint32_t w[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) w[k] = __builtin_bswap32(b[16u * c + k + 5u]);  // <= dword 84: inside the block
    if (c == 0) w[0] = (b[0] << 24) | ((b[1] & 0xFFu) << 16) | ((b[2] & 0xFFu) << 8) | (b[4] & 0xFFu);
    if (c == 4) {
      w[3] = (w[3] & 0xFFFF0000u) | 0x8000u;
#pragma unroll
      for (int k = 4; k < 15; ++k) w[k] = 0;
      w[15] = POW_MSG_BYTES * 8u;
    }
    compress(h, w);
  }
}

// The flags a block has on its own, given its digest h: POW_V_HASH and POW_V_WORK.
__device__ __forceinline__ uint32_t own_flags(const uint32_t* b, const uint32_t h[8], uint32_t diff) {
  uint32_t flags = 0;
  // ---- POW_V_HASH: the stored text, 64 characters from struct byte 290, then NUL ----
  uint32_t diffs = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint32_t d0 = b[72 + 2 * k], d1 = b[73 + 2 * k], d2 = b[74 + 2 * k];
    diffs |= ((d0 >> 16) | (d1 << 16)) ^ hex_of16(h[k] >> 16);
    diffs |= ((d1 >> 16) | (d2 << 16)) ^ hex_of16(h[k] & 0xFFFFu);
  }
  diffs |= b[88] & 0x00FF0000u;  // struct byte 354 = block_hash[64]
  if (diffs) flags |= POW_V_HASH;
  // ---- POW_V_WORK: on the computed digest ----
  if (leading_zero_bits(h) < diff) flags |= POW_V_WORK;
  return flags;
}

// The flags (POW_V_*) of the block at b, a raw struct in LDS.  has_parent: the
// struct behind it (b + BLK_DW) is its parent; it is read only then.
__device__ __forceinline__ uint32_t audit_block(const uint32_t* b, bool has_parent, uint32_t diff) {
  uint32_t h[8];
  hash_block(b, h);  // ---- block_to_hash ----
  uint32_t flags = own_flags(b, h, diff);
  // ---- POW_V_LINK, POW_V_INDEX: against the parent, the next block ----
  if (has_parent) {
    const uint32_t* const p = b + BLK_DW;
    if (b[0] - 1u != p[0]) flags |= POW_V_INDEX;
    // previous_block_hash (dwords 8..72) against the parent's block_hash
    // (dwords 72..136) as C strings of at most 256 bytes.  The two bytes in
    // front of either field count as equal and not NUL; the two behind as
    // NUL, which ends a string that fills its field.
    bool differ = false;
#pragma unroll 1
    for (uint32_t j = 0; j <= 64u; ++j) {
      uint32_t x = b[8u + j], y = p[72u + j];
      if (j == 0) { x |= 0xFFFFu; y |= 0xFFFFu; }
      if (j == 64u) { x &= 0xFFFFu; y &= 0xFFFFu; }
      const uint32_t nul = (x - 0x01010101u) & ~x & 0x80808080u;  // its lowest set bit marks x's first NUL
      if (nul) {
        const uint32_t upto = (2u << (uint32_t)__builtin_ctz(nul)) - 1u;  // the bytes up to and including it
        differ = ((x ^ y) & upto) != 0u;
        break;
      }
      if (x != y) {
        differ = true;
        break;
      }
    }
    if (differ) flags |= POW_V_LINK;
  }
  return flags;
}

}  // namespace powaudit
