// K8  pow_rand_kernel — one launch of pow_mine_rand: the lowest-trial search of
// K4-K6 (pow_walk_dev.h: expand, trial_of's hash, leave, winner) over the
// nonces the REFERENCE draws, 9 x rand() % 62 per trial (block.cpp:61-72) of
// glibc's TYPE_3 generator r[i] = r[i-31] + r[i-3] (pow_host.h), in place of
// the counter's nonces.  The key is the trial index relative to the launch.
//
// Layout.  A lane walks its runs of T trials (pow_rand_dev.h) in ascending
// order, so it stops as K4's does: at its first hit, at the end of the launch
// or once its next trial lies above the lowest solving trial published so far;
// that word only ever holds a trial that solved, so every trial below the
// answer is tested whatever the grid is.  Nobody waits for anybody.
//
// The generator.  A lane's state, 31 words, is a circular buffer in LDS laid
// out [word][lane] (a wave's 64 lanes read 64 consecutive dwords: no bank
// conflict), 31,744 bytes per workgroup.  A draw is two LDS reads, an add and
// a store.  The lanes reach their first trial from the host's state at the
// launch's, and hop from run to run, by the moves of pow_rand_dev.h.
#include "pow_rand_dev.h"
#include "pow_walk_dev.h"

using namespace powwalk;
using namespace powrand;

static_assert(sizeof(PowRandRec) == 64 && offsetof(PowRandIn, state) == sizeof(PowBatchCtl),
              "the host reads and writes the records as they are");
static_assert(WG == LANES, "the walk's workgroup is the tables'");

namespace {

struct RandLds {
  uint32_t st[NW][WG];      // column l: lane l's state, word i of it at row (head + i) % 31
  uint32_t xe[2 * NW + 2];  // the workgroup's state, extended to 61 words
  uint32_t tm[BLK_DW];      // the template
  uint32_t win_nonce[3];    // the last workgroup only
  WalkLds<false> walk;
};

__device__ __forceinline__ uint32_t wrap(uint32_t i) { return i >= NW ? i - NW : i; }

// The lane's next draw of rand(); its state moves on by one.
__device__ __forceinline__ uint32_t draw(uint32_t (&st)[NW][WG], uint32_t& head) {
  const uint32_t tid = threadIdx.x;
  const uint32_t v = st[head][tid] + st[wrap(head + 28u)][tid];
  st[head][tid] = v;
  head = wrap(head + 1u);
  return v >> 1;
}

// The lane's state moved by the polynomial coef(0..30): its column into registers, and back with the head at row 0.
template <class Coef>
__device__ __forceinline__ void apply(uint32_t (&st)[NW][WG], uint32_t& head, Coef coef) {
  const uint32_t tid = threadIdx.x;
  uint32_t s[NW];
#pragma unroll
  for (uint32_t j = 0; j < NW; ++j) s[j] = st[wrap(head + j)][tid];
  powrand::apply(s, coef);
#pragma unroll
  for (uint32_t j = 0; j < NW; ++j) st[j][tid] = s[j];
  head = 0u;
}

}  // namespace

__global__ __launch_bounds__(256) void pow_rand_kernel(const PowRandLaunch L, const PowRandIn* __restrict__ in,
                                                       const uint32_t* __restrict__ tab, PowBatchCtl* ctl,
                                                       PowChainSlot* slots, uint32_t* slot_nonce,
                                                       PowRandRec* __restrict__ rec) {
  __shared__ RandLds sh;
  const uint32_t tid = threadIdx.x;
  const uint32_t part = blockIdx.x;
  const uint32_t* const tmpl = (const uint32_t*)&in->tmpl;
  if (tid < BLK_DW) sh.tm[tid] = tmpl[tid];
  if (tid < NW) sh.xe[tid] = in->state[tid];
  if (tid < 8u) sh.walk.win_digest[tid] = 0u;  // the record's digest where the launch holds no solution
  if (tid < 3u) sh.win_nonce[tid] = 0u;
  if (tid == 0) {
    sh.walk.wg_min = ~0ull;
    sh.walk.wg_trials = 0ull;
  }
  const uint32_t thr = in->thr;
  __syncthreads();
  expand(sh.walk.msg0, sh.walk.kw, sh.tm, 5u,
         (sh.tm[0] << 24) | ((sh.tm[1] & 0xFFu) << 16) | ((sh.tm[2] & 0xFFu) << 8) | (sh.tm[4] & 0xFFu));

  // ---- the workgroup's state: the launch's moved by x^(9 T 256 part) ----
  group_move(sh.xe, tab + NW * LANES + part * NW);  // its last barrier also: msg0 and kw are expanded

  // ---- the lane's: that moved by x^(9 T tid) ----
#pragma unroll
  for (uint32_t j = 0; j < NW; ++j) sh.st[j][tid] = sh.xe[j];
  uint32_t head = 0u;
  apply(sh.st, head, [&](uint32_t i) { return tab[i * LANES + tid]; });

  // ---- the walk ----
  Hit me;
  me.key = ~0ull;
#pragma unroll
  for (int k = 0; k < 8; ++k) me.digest[k] = 0u;
  me.trials = 0;
  uint32_t nonce_w[3] = {0u, 0u, 0u};
  const uint32_t hop_by = hop_of(L.nwg, L.run);
  uint32_t rel = first_rel(part, L.run), in_run = 0u;
  bool go = rel < L.count;
  while (go) {
    uint32_t c[9], h[8];
    const auto chars = [&](uint32_t (&nine)[9]) {  // gen_random_nonce, block.cpp:61-72
#pragma unroll
      for (int i = 0; i < 9; ++i) nine[i] = c[i] = digit_char(draw(sh.st, head) % 62u);
    };
    trial_of(chars, sh.walk.msg0, sh.walk.kw, h);
    ++me.trials;
    if (h[0] <= thr) {
      me.key = rel;
#pragma unroll
      for (int k = 0; k < 8; ++k) me.digest[k] = h[k];
      nonce_w[0] = (c[0] << 24) | (c[1] << 16) | (c[2] << 8) | c[3];
      nonce_w[1] = (c[4] << 24) | (c[5] << 16) | (c[6] << 8) | c[7];
      nonce_w[2] = c[8];
      atomicMin(&ctl->min_rel, me.key);
      break;  // the lane's later trials are higher
    }
    ++rel;
    const bool hop = ++in_run == L.run;
    if (hop) {
      in_run = 0u;
      rel += hop_by;
    }
    go = rel < L.count && rel <= load_agent(&ctl->min_rel);
    if (go && hop) apply(sh.st, head, [&](uint32_t i) { return in->step[i]; });
  }
  if (me.key != ~0ull) atomicMin(&sh.walk.wg_min, me.key);
  if (me.trials) atomicAdd(&sh.walk.wg_trials, (unsigned long long)me.trials);
  __syncthreads();
  // The workgroup's lowest hit: its nonce words beside its slot, by the lane
  // that writes the slot and before that lane's fence in leave().
  if (me.key != ~0ull && me.key == sh.walk.wg_min) {
#pragma unroll
    for (int k = 0; k < 3; ++k) slot_nonce[3u * part + k] = nonce_w[k];
  }
  const Exit out = leave(sh.walk, me, slots + part, &ctl->exits, L.nwg);
  if (!out.last) return;

  // ---- the last workgroup out writes the launch's record ----
  const unsigned long long best = winner(sh.walk, &ctl->min_rel, slots, L.nwg);
  for (uint32_t s = tid; s < L.nwg; s += WG) {
    if (best != ~0ull && load_agent(&slots[s].rel) == best) {  // exactly one slot
#pragma unroll
      for (int k = 0; k < 3; ++k) sh.win_nonce[k] = load_agent(&slot_nonce[3u * s + k]);
    }
  }
  __syncthreads();
  if (tid == 0) {
    rec->rel = best;
#pragma unroll
    for (int k = 0; k < 8; ++k) rec->digest[k] = sh.walk.win_digest[k];
    rec->trials = out.trials;
#pragma unroll
    for (int k = 0; k < 3; ++k) rec->nonce_w[k] = sh.win_nonce[k];
    rec->pad = 0u;
  }
}

// One pass of the grid is nwg x 256 x run <= 2^26 trials, so a lane's trial
// index stays below 2^27.  slots: nwg entries; slot_nonce: 3 x nwg words; tab:
// POW_RAND_TAB_WORDS words (pow_rand_tables of L.run).
hipError_t pow_launch_rand(hipStream_t stream, const PowRandLaunch& L, const PowRandIn* in, const uint32_t* tab,
                           PowBatchCtl* ctl, PowChainSlot* slots, uint32_t* slot_nonce, PowRandRec* rec) {
  if (L.nwg == 0 || L.nwg > POW_RAND_MAX_WG || L.run == 0 || L.run > POW_RAND_MAX_RUN || L.count == 0 ||
      L.count > (1u << 26))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(pow_rand_kernel, dim3(L.nwg), dim3(WG), 0, stream, L, in, tab, ctl, slots, slot_nonce, rec);
  return hipGetLastError();
}
