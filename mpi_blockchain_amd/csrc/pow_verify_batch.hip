// K7  pow_verify_batch_kernel — the audit of many independent chains in one
// pass (pow_verify_chains): K3's audit (pow_audit_dev.h) of every block of a
// buffer that holds the chains back to back, each tip first, with a verdict
// per chain.
//
// The frame is K3's: one lane per block, workgroups of 64 (one wave), the
// wave's 64 raw structs plus one halo block in LDS (65 x 552 B = 35,880 B).
// The concatenation is contiguous, so the tiling does not know the chains.
//
// What is new is the segmentation.  offs is the exclusive prefix sum of the
// chains' lengths (n_chains + 1 words, offs[n_chains] = all blocks): chain c
// is the global positions [offs[c], offs[c + 1]).  A live lane finds its
// chain by binary search for its global position g: the lowest c with
// offs[c + 1] > g, which steps over empty chains (equal neighbouring
// offsets: an empty chain's offs[c + 1] is no greater than its offs[c] <= g,
// so it is never the answer) in at most 21 dependent loads, against 320
// compression rounds.  The block has a parent exactly when g + 1 is still
// inside its chain; only then is the struct behind it read, the LDS neighbour
// or the halo for lane 63.  The host gives every tile that does not end the
// buffer a halo, so the parent of a chain that goes on is always present; the
// halo of a chain's last block is a stranger and is not looked at.
//
// Verdicts: first_bad[c] (atomic min of the position within the chain; the
// host resets it to all-ones) and n_bad[c] (atomic add; reset to zero), both
// accumulated over the call's launches.  Only flagged lanes issue atomics: a
// batch of valid chains issues none.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pow_audit_dev.h"
#include "pow_ctx.h"

using namespace powaudit;

// blocks: the n_avail structs of a host tile, of which the first n_check are
// verified; block n_check (present iff n_avail > n_check) is only the parent
// of block n_check - 1, if that one has a parent.  base: the global position
// of the tile's first block.  K3's budget: at most 64 VGPRs, no scratch, the
// LDS of the tile only (pow_node's receive context runs beside K1).
__global__ __launch_bounds__(64) __attribute__((amdgpu_num_vgpr(64))) void pow_verify_batch_kernel(
    const uint32_t* __restrict__ blocks, uint32_t n_check, uint32_t n_avail, uint32_t base,
    const uint32_t* __restrict__ offs, uint32_t n_chains, uint32_t diff, uint8_t* __restrict__ status,
    uint32_t* __restrict__ first_bad, uint32_t* __restrict__ n_bad) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[TILE_LDS_DW];
  const uint32_t lane = threadIdx.x;
  const uint32_t first = blockIdx.x * TILE;
  load_tile(lds, blocks, first, n_avail, lane);
  __syncthreads();
  const uint32_t t = first + lane;
  if (t >= n_check) return;  // dead lanes neither search nor write
  const uint32_t g = base + t;
  // The lowest c with offs[c + 1] > g; offs[n_chains] > g bounds the search.
  uint32_t lo = 0, hi = n_chains - 1u;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (offs[mid + 1u] > g) hi = mid; else lo = mid + 1u;
  }
  const uint32_t c = lo;
  const uint32_t flags = audit_block(lds + lane * BLK_DW, g + 1u < offs[c + 1u], diff);
  status[t] = (uint8_t)flags;
  if (flags) {
    atomicMin(&first_bad[c], g - offs[c]);
    atomicAdd(&n_bad[c], 1u);
  }
}

hipError_t pow_launch_verify_batch(uint32_t n_check, uint32_t n_avail, uint32_t base, unsigned diff,
                                   hipStream_t stream, const uint32_t* blocks, const uint32_t* offs,
                                   uint32_t n_chains, uint8_t* status, uint32_t* first_bad, uint32_t* n_bad) {
  if (n_check == 0 || n_chains == 0) return hipSuccess;
  hipLaunchKernelGGL(pow_verify_batch_kernel, dim3((n_check + TILE - 1) / TILE), dim3(TILE), 0, stream, blocks,
                     n_check, n_avail, base, offs, n_chains, (uint32_t)diff, status, first_bad, n_bad);
  return hipGetLastError();
}
