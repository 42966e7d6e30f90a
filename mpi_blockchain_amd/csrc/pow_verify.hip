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
// The audit of one block and the copy of the tile are pow_audit_dev.h, shared
// with K7 (pow_verify_batch.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pow_audit_dev.h"
#include "pow_ctx.h"

using namespace powaudit;

// blocks: n_avail structs, of which the first n_check are verified; block
// n_check (present iff n_avail > n_check) is only the parent of block
// n_check - 1.  res is {lowest flagged index (min), flagged blocks (sum)}.
// At most 64 VGPRs, as K2: beside a running K1 (7 of a SIMD's 8 wave slots of 64
// VGPRs taken) that is what is left.  Its LDS, not its registers, bounds its
// own occupancy: four workgroups per CU beside nothing else.
__global__ __launch_bounds__(64) __attribute__((amdgpu_num_vgpr(64))) void pow_verify_kernel(
    const uint32_t* __restrict__ blocks, uint32_t n_check, uint32_t n_avail, uint32_t diff,
    uint8_t* __restrict__ status, PowVerifyRes* __restrict__ res) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[TILE_LDS_DW];
  const uint32_t lane = threadIdx.x;
  const uint32_t first = blockIdx.x * TILE;
  load_tile(lds, blocks, first, n_avail, lane);
  __syncthreads();
  const uint32_t g = first + lane;
  uint32_t flags = 0;
  if (g < n_check) {
    flags = audit_block(lds + lane * BLK_DW, g + 1u < n_avail, diff);
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
