// K3  pow_verify_kernel — the audit of a chain of blocks (pow_verify_chain):
// block_to_hash (block.cpp:74-88) of every block, compared with its stored
// block_hash; the proof of work of the computed digest (block.cpp:91-96); and
// the link and index checks of check_chain (node.cpp:117-125), fused in one
// pass over the raw 552-byte structs.  The result is a verdict (one status
// byte per block, the lowest flagged index and the flagged count), not digests.
//
// One lane per block, workgroups of 64 (one wave), as K2.  The workgroup
// copies its 64 blocks plus one halo block (the next tile's first: the parent
// the last lane links to) into LDS with coalesced 16-byte global loads:
// 65 x 552 B = 35,880 B.
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
// The kernel's time is the 320 compression rounds, not its ~100 LDS reads.
//
// The stored hashes sit at struct byte 290 (block_hash) and 34
// (previous_block_hash): both 2 bytes past a dword, so the link check compares
// whole dwords of the two fields (child's dword 8 + j with the parent's dword
// 72 + j), and the hex check shifts the stored text by 16 bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pow_ctx.h"
#include "sha256_dev.h"

using namespace powdev;

namespace {

constexpr uint32_t BLK_DW = sizeof(pow_block) / 4;  // 138
constexpr uint32_t TILE = 64;                       // blocks per workgroup (one per lane)
static_assert(sizeof(pow_block) == 552 && offsetof(pow_block, nonce) == 24 &&
                  offsetof(pow_block, previous_block_hash) == 34 && offsetof(pow_block, block_hash) == 290,
              "the kernel's word offsets are those of the reference's struct Block");

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

}  // namespace

// blocks: n_avail structs, of which the first n_check are verified; block
// n_check (present iff n_avail > n_check) is only the parent of block
// n_check - 1.  res is {lowest flagged index (min), flagged blocks (sum)}.
// At most 64 VGPRs, as K2: beside a running K1 (7 of a SIMD's 8 wave slots of 64
// VGPRs taken) that is what is left.  Its LDS, not its registers, bounds its
// own occupancy: four workgroups per CU beside nothing else.
__global__ __launch_bounds__(64) __attribute__((amdgpu_num_vgpr(64))) void pow_verify_kernel(
    const uint32_t* __restrict__ blocks, uint32_t n_check, uint32_t n_avail, uint32_t diff,
    uint8_t* __restrict__ status, PowVerifyRes* __restrict__ res) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[(TILE + 1) * BLK_DW];
  const uint32_t lane = threadIdx.x;
  const uint32_t first = blockIdx.x * TILE;
  {
    // 64 blocks are 35,328 B, a multiple of 16, so every workgroup's source
    // is 16-byte aligned; the copy's length (a multiple of 8) may end on a
    // half vector, which goes as two dwords.
    const uint32_t nb = min(TILE + 1u, n_avail - first);
    const uint32_t ndw = nb * BLK_DW, nvec = ndw >> 2;
    const uint32_t* const src = blocks + (size_t)first * BLK_DW;
    const uint4* const src4 = (const uint4*)src;
    uint4* const lds4 = (uint4*)lds;
    for (uint32_t v = lane; v < nvec; v += 64u) lds4[v] = src4[v];
    if (lane < (ndw & 3u)) lds[4u * nvec + lane] = src[4u * nvec + lane];
  }
  __syncthreads();
  const uint32_t g = first + lane;
  const bool live = g < n_check;
  uint32_t flags = 0;
  if (live) {
    const uint32_t* const b = lds + lane * BLK_DW;
    // ---- block_to_hash ----
    uint32_t h[8];
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
    // ---- POW_V_LINK, POW_V_INDEX: against the parent, the next block ----
    if (g + 1u < n_avail) {
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
    status[g] = (uint8_t)flags;
  }
  // One atomic min and one atomic add per wave that holds a flagged block.
  const unsigned long long bad = __ballot(flags != 0u);
  if (bad != 0ull && lane == 0) {
    atomicMin(&res->first_bad, first + (uint32_t)__builtin_ctzll(bad));
    atomicAdd(&res->n_bad, (uint32_t)__builtin_popcountll(bad));
  }
}

hipError_t pow_launch_verify(uint32_t n_check, uint32_t n_avail, unsigned diff, hipStream_t stream,
                             const uint32_t* blocks, uint8_t* status, PowVerifyRes* res) {
  if (n_check == 0) return hipSuccess;
  hipLaunchKernelGGL(pow_verify_kernel, dim3((n_check + TILE - 1) / TILE), dim3(TILE), 0, stream, blocks, n_check,
                     n_avail, (uint32_t)diff, status, res);
  return hipGetLastError();
}
