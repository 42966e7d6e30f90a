// K9  pow_seed_kernel — one launch of pow_find_seed: K8's walk over the nonces
// the REFERENCE draws (pow_rand.hip, pow_host.h), without the hash.  Every
// (seed, trial) pair of the launch's tile of seeds and slice of trials is
// compared with up to 64 target nonces, and every match is recorded: the search
// is exhaustive, nothing stops early and nobody waits for anybody.  The
// generator's moves and the layout of the runs are pow_rand_dev.h's.
//
// Seeding.  blockIdx.x = (seed position within the tile, part): each seed has
// nwg workgroups.  One lane of each restates pow_rand_seed (pow_host.cpp): the
// 30 Lehmer steps and the 310 discarded ones, in registers.  The workgroup moves
// that state to the slice's first trial by the launch's polynomial (the same
// for every seed), then on by the tables.
//
// The walk.  With no SHA-256 in the lane the 31-word state is 31 VGPRs.  One
// iteration is 31 trials = 279 draws, fully unrolled: lcm(9, 31) = 279, so the
// circular head and the trial boundary are compile-time constants in every
// draw, a draw is one add in place, and no register is indexed dynamically.
// Hence T is a multiple of 31.  A trial's first two digits go through a 62 x
// 62-bit table in LDS, and where some target begins with them its third and
// fourth through a second one; only where both pass are the other digits made
// and the target list walked.  One table alone lets 64 targets through in 1.7 %
// of a lane's trials, which is two of three trials of a wave of 64, and the wave
// pays for the list whenever one lane walks it: the second table brings that
// down to 1.8 % of a wave's trials.  A lane walks whole iterations and never
// tests the slice's end per trial: the bound is applied where a match is recorded.
#include "pow_rand_dev.h"

using namespace powrand;

namespace {

struct SeedLds {
  uint32_t xe[2 * NW + 2];                 // the workgroup's state, extended to 61 words
  unsigned long long pair[62];             // PowSeedIn::pair
  unsigned long long pair2[62];            // PowSeedIn::pair2
  uint32_t tgt[POW_SEED_MAX_TARGETS][2];   // PowSeedIn::tgt
};

// pow_rand_seed: r[0..30] by the 16807 Lehmer step (signed, C division, the
// + 2^31 - 1 fix-up), r[31..33] = r[0..2], r[i] = r[i-31] + r[i-3] up to r[343];
// the state is r[313..343].  r lives in a circular window of 31 registers:
// slot i % 31 holds r[i - 31] until r[i] replaces it, and 313 % 31 = 3.
__device__ __forceinline__ void seed_state(uint32_t seed, uint32_t (&x)[NW]) {
  uint32_t r[NW];
  r[0] = seed ? seed : 1u;
#pragma unroll
  for (uint32_t i = 1; i < NW; ++i) {
    const int32_t w = (int32_t)r[i - 1u];
    const int32_t hi = w / 127773, lo = w - hi * 127773;
    long long v = 16807ll * lo - 2836ll * hi;
    if (v < 0) v += 2147483647;
    r[i] = (uint32_t)v;
  }
#pragma unroll
  for (uint32_t i = 34; i < 344; ++i) r[i % NW] += r[(i - 3u) % NW];
#pragma unroll
  for (uint32_t j = 0; j < NW; ++j) x[j] = r[(j + 3u) % NW];
}

// A trial that passed both tables: the target list, and a record
// for every target that equals all nine, if the trial lies inside the slice.
__device__ __forceinline__ void compare(const SeedLds& sh, uint32_t n_targets, uint32_t w0, uint32_t w1, uint32_t pos,
                                        uint32_t rel, uint32_t count, PowSeedOut* out) {
  for (uint32_t k = 0; k < n_targets; ++k) {
    if (sh.tgt[k][0] != w0 || sh.tgt[k][1] != w1 || rel >= count) continue;
    const uint32_t slot = atomicAdd(&out->n, 1u);
    if (slot < POW_SEED_DEV_CAP) {  // the host fails the call above it
      out->rec[slot].pos = pos;
      out->rec[slot].target = k;
      out->rec[slot].rel = rel;
    }
  }
}

}  // namespace

__global__ __launch_bounds__(256) void pow_seed_kernel(const PowSeedLaunch L, const PowSeedIn* __restrict__ in,
                                                       const uint32_t* __restrict__ tab, PowSeedOut* out) {
  __shared__ SeedLds sh;
  const uint32_t tid = threadIdx.x;
  const uint32_t local = blockIdx.x / L.nwg;  // the seed within the tile
  const uint32_t part = blockIdx.x - local * L.nwg;
  const uint32_t pos = L.pos_base + local;
  const uint32_t n_targets = min(in->n_targets, (uint32_t)POW_SEED_MAX_TARGETS);
  if (tid < 62u) sh.pair[tid] = in->pair[tid];
  if (tid < 62u) sh.pair2[tid] = in->pair2[tid];
  if (tid < 2u * POW_SEED_MAX_TARGETS) (&sh.tgt[0][0])[tid] = (&in->tgt[0][0])[tid];

  // ---- the seed's state at draw 0, then at the slice's first trial, then at the workgroup's ----
  if (tid == 0) {
    uint32_t s0[NW];
    seed_state(L.seed_first + pos, s0);
#pragma unroll
    for (uint32_t j = 0; j < NW; ++j) sh.xe[j] = s0[j];
  }
  group_move(sh.xe, in->jump);
  group_move(sh.xe, tab + NW * LANES + part * NW);  // table B's x^(9 T 256 part)

  // ---- the lane's: that moved by table A's x^(9 T tid) ----
  uint32_t x[NW];
#pragma unroll
  for (uint32_t j = 0; j < NW; ++j) x[j] = sh.xe[j];
  apply(x, [&](uint32_t i) { return tab[i * LANES + tid]; });

  // ---- the walk ----
  const uint32_t iters = L.run / NW, hop_by = hop_of(L.nwg, L.run);
  uint32_t rel = first_rel(part, L.run);
  while (rel < L.count) {
#pragma unroll 1
    for (uint32_t it = 0; it < iters; ++it) {
#pragma unroll
      for (uint32_t t = 0; t < NW; ++t) {  // 31 trials: the head is back at 0 after them
#pragma unroll
        for (uint32_t i = 0; i < 9u; ++i) {  // gen_random_nonce's nine draws, block.cpp:61-72
          const uint32_t h = (9u * t + i) % NW;
          x[h] += x[(h + 28u) % NW];
        }
        // draw i of the trial stands at x[(9 t + i) % 31] until 31 draws later
        const uint32_t d0 = (x[(9u * t) % NW] >> 1) % 62u;
        const uint32_t d1 = (x[(9u * t + 1u) % NW] >> 1) % 62u;
        if ((sh.pair[d0] >> d1) & 1ull) {
          const uint32_t d2 = (x[(9u * t + 2u) % NW] >> 1) % 62u;
          const uint32_t d3 = (x[(9u * t + 3u) % NW] >> 1) % 62u;
          if (!((sh.pair2[d2] >> d3) & 1ull)) continue;
          uint32_t w0 = (((((d0 << 6) | d1) << 6) | d2) << 6) | d3, w1 = 0u;
          w0 = (w0 << 6) | ((x[(9u * t + 4u) % NW] >> 1) % 62u);
#pragma unroll
          for (uint32_t i = 5; i < 9u; ++i) w1 = (w1 << 6) | ((x[(9u * t + i) % NW] >> 1) % 62u);
          compare(sh, n_targets, w0, w1, pos, rel + t, L.count, out);
        }
      }
      rel += NW;
    }
    rel += hop_by;
    if (rel < L.count) apply(x, [&](uint32_t i) { return in->step[i]; });
  }
}

// A pass of the grid is nwg x 256 x run < 2^26 trials and the slice at most
// 2^26, so a lane's trial index stays below 2^27.  tab: POW_RAND_TAB_WORDS words
// (pow_rand_tables of L.run).
hipError_t pow_launch_seed(hipStream_t stream, const PowSeedLaunch& L, const PowSeedIn* in, const uint32_t* tab,
                           PowSeedOut* out) {
  const uint32_t j = L.run / NW;
  if (L.nwg == 0 || L.nwg > POW_RAND_MAX_WG || L.run == 0 || L.run % NW != 0 || (j & (j - 1u)) != 0 || j > 32u ||
      L.count == 0 || L.count > (1u << 26) || L.n_seeds == 0 || (uint64_t)L.n_seeds * L.nwg > (1u << 16) ||
      (uint64_t)L.pos_base + L.n_seeds > POW_SEED_MAX_SEEDS)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(pow_seed_kernel, dim3(L.n_seeds * L.nwg), dim3(LANES), 0, stream, L, in, tab, out);
  return hipGetLastError();
}
