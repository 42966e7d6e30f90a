// K6  pow_race_kernel — one height of pow_mine_race per launch: N rival miners
// (node.cpp:292-302: every rank refreshes its own template on the same tip),
// each with K4's template refresh and pow_walk_dev.h's search, under ONE
// minimum shared by all of them, and K4's success tail for the winner alone.
//
// A launch reads the block before it (`prev`) and writes the winner's sealed
// block (`dst`) and the height's record; the launches of a batch are queued on
// one stream as K4's are.
//
// The grid is flat: workgroup w serves rival w % R as part w / R of that
// rival's nwg_r workgroups, so the workgroups that start first hold every
// rival's lowest counters.  A workgroup belongs to one rival: it reads the
// parent and its rival's owner and created_at (device arrays that went up once
// per batch) for word 0 of the message.  Only word 0 differs between two
// rivals, and only in two bytes: rivals whose owners and created_at agree in
// their low bytes have identical digests.
//
// The race: a pair (relative counter rel, rival r) has the key rel << 8 | r,
// and the winner of the height is the solving pair with the lowest key: the
// lowest counter, ties to the lowest position.  All rivals' lanes share one
// minimum word and one exit word per launch and read the minimum early, so a
// height costs about the trials of one solo block, not R times that.  The last
// workgroup of the whole grid seals the block with the winner's owner and
// created_at and writes the record.  A height nobody solves raises `stop`.
#include "pow_walk_dev.h"

using namespace powwalk;

static_assert(POW_RACE_MAX_RIVALS == 256, "a key carries the rival in its low 8 bits");
static_assert(sizeof(PowRaceRec) == 16 && sizeof(PowSealCtl) == 32, "the host reads the records as they are");

__global__ __launch_bounds__(256) void pow_race_kernel(const PowRaceLaunch L, const uint32_t* __restrict__ prev,
                                                       uint32_t* __restrict__ dst, const PowRaceIn* __restrict__ in,
                                                       PowSealCtl* ctl, PowChainSlot* slots,
                                                       PowRaceRec* __restrict__ recs) {
  __shared__ SealerLds<true> sh;
  const uint32_t part = blockIdx.x / L.n_rivals;
  const uint32_t r = blockIdx.x - part * L.n_rivals;
  const uint32_t nwg = L.nwg_r * L.n_rivals;
  const uint64_t* const created_at = in->created_at + (size_t)L.height * L.n_rivals;
  if (!load_parent(sh.par, prev, ctl)) return;
  const auto word0 = [&] {
    return ((sh.par[0] + 1u) << 24) | ((in->owner[r] & 0xFFu) << 16) | ((L.diff & 0xFFu) << 8) |
           ((uint32_t)created_at[r] & 0xFFu);
  };
  const Hit me = walk(sh.walk, L.w, sh.par, 69u, word0, part, L.nwg_r, &ctl->min_key, [r](uint64_t rel) { return (rel << 8) | r; });
  const Exit out = leave(sh.walk, me, slots + blockIdx.x, &ctl->exits, nwg);
  if (!out.last) return;

  // ---- the last workgroup out seals the winner's block ----
  const unsigned long long best = winner(sh.walk, &ctl->min_key, slots, nwg);
  if (!close_launch(ctl, out.trials, best)) return;
  const uint32_t win = (uint32_t)(best & 0xFFull);
  const uint32_t best_rel = (uint32_t)(best >> 8);
  if (threadIdx.x == 0) {
    PowRaceRec* const rec = recs + L.height;
    rec->rel = best_rel;
    rec->winner = win;
    rec->pad = 0u;
  }
  seal(sh, L.w.base_digit, best_rel, in->owner[win], L.diff, created_at[win], dst, ctl);
}

// L.n_rivals x L.nwg_r workgroups: the caller keeps the product below POW_RACE_MAX_WG
// and at or below the slots it allocated.
hipError_t pow_launch_race(hipStream_t stream, const PowRaceLaunch& L, const uint32_t* prev, uint32_t* dst,
                           const PowRaceIn* in, PowSealCtl* ctl, PowChainSlot* slots, PowRaceRec* rec) {
  if (L.n_rivals == 0 || L.n_rivals > POW_RACE_MAX_RIVALS || L.nwg_r == 0 || L.height >= POW_RACE_MAX_BATCH ||
      (uint64_t)L.n_rivals * L.nwg_r >= POW_RACE_MAX_WG)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(pow_race_kernel, dim3(L.n_rivals * L.nwg_r), dim3(WG), 0, stream, L, prev, dst, in, ctl, slots, rec);
  return hipGetLastError();
}
