// K4  pow_chain_kernel — one block of pow_mine_chain per launch: the template
// refresh of node.cpp:292-299, the lowest-counter search of pow_mine and the
// success tail of node.cpp:311-318, with no host step between two blocks.
// The search, the leaving and the seal are pow_walk_dev.h's.
//
// A launch reads the block before it (`prev`: the caller's parent for the
// first launch of a batch, else the block the launch before it sealed) and
// writes its own sealed block (`dst`).  The launches of a batch are queued on
// one stream, so a launch sees what its predecessor wrote (kernel boundaries
// order them); inside a launch `prev` is only read and `dst` only written.
//
// The grid is one template's: workgroup w is part w of L.nwg, the key is the
// relative counter, and word 0 of the message is the refreshed template's
// (index + 1 and the launch's owner, difficulty and created_at).  The host
// keeps the grid at one workgroup per CU or below, so every workgroup starts
// at once and none reads the minimum before its first trial.  A window
// without a solution raises `stop`.
#include "pow_walk_dev.h"

using namespace powwalk;

__global__ __launch_bounds__(256) void pow_chain_kernel(const PowChainLaunch L, const uint32_t* __restrict__ prev,
                                                        uint32_t* __restrict__ dst, PowSealCtl* ctl,
                                                        PowChainSlot* slots) {
  __shared__ SealerLds<false> sh;
  if (!load_parent(sh.par, prev, ctl)) return;
  const auto word0 = [&] {
    return ((sh.par[0] + 1u) << 24) | ((L.owner & 0xFFu) << 16) | ((L.diff & 0xFFu) << 8) | ((uint32_t)L.created_at & 0xFFu);
  };
  const Hit me = walk(sh.walk, L.w, sh.par, 69u, word0, blockIdx.x, L.nwg, &ctl->min_key, [](uint64_t rel) { return rel; });
  const Exit out = leave(sh.walk, me, slots + blockIdx.x, &ctl->exits, L.nwg);
  if (!out.last) return;

  // ---- the last workgroup out seals the block ----
  const unsigned long long best = winner(sh.walk, &ctl->min_key, slots, L.nwg);
  if (!close_launch(ctl, out.trials, best)) return;
  seal(sh, L.w.base_digit, (uint32_t)best, L.owner, L.diff, L.created_at, dst, ctl);
}

hipError_t pow_launch_chain(hipStream_t stream, const PowChainLaunch& L, const uint32_t* prev, uint32_t* dst,
                            PowSealCtl* ctl, PowChainSlot* slots) {
  if (L.nwg == 0 || L.nwg > POW_WALK_MAX_WG) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pow_chain_kernel, dim3(L.nwg), dim3(WG), 0, stream, L, prev, dst, ctl, slots);
  return hipGetLastError();
}
