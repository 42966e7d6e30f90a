// K5  pow_batch_kernel — one tile of pow_mine_batch per launch: many
// independent templates, each with its own lowest-counter search
// (pow_walk_dev.h's walk), over the raw 552-byte structs as K3 reads them.
//
// The grid is flat and one-dimensional (gridDim.y stops at 65,535): workgroup
// w serves template w / nwg_t as part w % nwg_t of that template's nwg_t
// workgroups.  A workgroup belongs to one template: it copies the template's
// 138 dwords into LDS and hashes the struct as it stands (word 0 and the
// previous_block_hash are its own: base 5), with the relative counter as the
// key and the template's own control words, slots and exit count.  A grid may
// be many times what the chip holds, so the walk reads the minimum early.
// The last of a template's workgroups to leave writes the template's result
// record from the slots; the host resets the control words per tile and seals
// the blocks.
#include "pow_walk_dev.h"

using namespace powwalk;

static_assert(sizeof(PowBatchRec) == 48 && sizeof(PowBatchCtl) == 16, "the host reads the records as they are");

__global__ __launch_bounds__(256) void pow_batch_kernel(const PowBatchLaunch L, const uint32_t* __restrict__ tmpls,
                                                        PowBatchCtl* ctls, PowChainSlot* slots,
                                                        PowBatchRec* __restrict__ recs) {
  __shared__ uint32_t tm[BLK_DW];  // the template
  __shared__ WalkLds<true> sh;
  const uint32_t tid = threadIdx.x;
  const uint32_t t = blockIdx.x / L.nwg_t;
  const uint32_t part = blockIdx.x - t * L.nwg_t;
  PowBatchCtl* const ctl = ctls + t;
  PowChainSlot* const tslots = slots + (size_t)t * L.nwg_t;
  if (tid < BLK_DW) tm[tid] = tmpls[(size_t)t * BLK_DW + tid];
  if (tid < 8u) sh.win_digest[tid] = 0u;  // the record's digest where the window holds no solution
  const auto word0 = [&] { return (tm[0] << 24) | ((tm[1] & 0xFFu) << 16) | ((tm[2] & 0xFFu) << 8) | (tm[4] & 0xFFu); };
  const Hit me = walk(sh, L.w, tm, 5u, word0, part, L.nwg_t, &ctl->min_rel, [](uint64_t rel) { return rel; });
  const Exit out = leave(sh, me, tslots + part, &ctl->exits, L.nwg_t);
  if (!out.last) return;

  // ---- the template's last workgroup out writes its record ----
  const unsigned long long best = winner(sh, &ctl->min_rel, tslots, L.nwg_t);
  __syncthreads();
  if (tid == 0) {
    PowBatchRec* const rec = recs + t;
    rec->rel = best;
#pragma unroll
    for (int k = 0; k < 8; ++k) rec->digest[k] = sh.win_digest[k];
    rec->trials = out.trials;
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
