// The plans of pow_mine_chain's and pow_mine_batch's fused paths
// (pow_chain_plan, pow_batch_plan, csrc/pow_host.cpp) on the CPU: linked with
// pow_host.cpp alone and run under AddressSanitizer + UndefinedBehaviorSanitizer
// by tests/test_chain_host.py.  Over every difficulty, window, chip size, lanes
// switch, override and template count of the lists below it checks what
// pow_host.h promises and the two calls rely on for their slots, their tile
// buffers and their watchdog, and the shapes the shipped library runs.
#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "pow_host.h"

int main() {
  const uint32_t cus[] = {1, 32, 256};
  const uint64_t windows[] = {1, 2, 255, 256, 257, 700, 1ull << 12, 1ull << 16, (1ull << 16) + 1, 1ull << 24, 1ull << 30,
                              (1ull << 32) - 1, 1ull << 32};
  const unsigned lanes[] = {0, 2, 8};
  const int batch_lanes[] = {-1, 0, 2, 8};
  const unsigned overrides[] = {0, 1, 64};
  const unsigned tile_overrides[] = {0, 1, 64, 16384};
  const uint64_t counts[] = {1, 2, 64, 1024, 1ull << 24};
  long plans = 0, failed = 0;
  for (unsigned d = 0; d <= 32; ++d)
    for (uint32_t cu : cus)
      for (uint64_t w : windows) {
        for (unsigned ll : lanes)
          for (unsigned ov : overrides) {
            const PowChainPlan p = pow_chain_plan(d, w, cu, ll, ov);
            ++plans;
            bool ok = p.nwg >= 1 && p.nwg <= std::max(1u, cu);
            ok = ok && (uint64_t)(p.nwg - 1) * 256 < w;  // no workgroup starts past the window
            ok = ok && p.batch >= 1 && p.batch <= POW_CHAIN_MAX_BATCH;
            if (ov) ok = ok && p.batch == ov;
            if (!ok) {
              if (++failed <= 20)
                printf("chain d=%u cu=%u window=%llu lanes_log2=%u override=%u: nwg=%u batch=%u\n", d, cu,
                       (unsigned long long)w, ll, ov, p.nwg, p.batch);
            }
          }
        for (int ll : batch_lanes)
          for (unsigned ov : tile_overrides)
            for (uint64_t n : counts) {
              const PowBatchPlan p = pow_batch_plan(d, n, w, cu, ll, ov);
              ++plans;
              bool ok = p.nwg_t >= 1 && p.nwg_t <= std::max(1u, cu);
              ok = ok && p.tile >= 1 && p.tile <= POW_BATCH_MAX_TILE;
              ok = ok && (uint64_t)p.tile * p.nwg_t <= POW_BATCH_MAX_WG;
              // an override is capped like the planned tile: no exception for it
              ok = ok && (p.tile == 1 || (uint64_t)p.tile * w <= (1ull << 38));
              ok = ok && (p.nwg_t == 1 || (uint64_t)(p.nwg_t - 1) * 256 < w);
              if (ov) ok = ok && p.tile <= ov;
              if (!ok) {
                if (++failed <= 20)
                  printf("batch d=%u n=%llu cu=%u window=%llu lanes_log2=%d override=%u: nwg_t=%u tile=%u\n", d,
                         (unsigned long long)n, cu, (unsigned long long)w, ll, ov, p.nwg_t, p.tile);
              }
            }
      }
  // The shipped shapes on 256 CUs, by hand from the plans' statements.  Chain,
  // lanes for four times 2^d trials: d = 18 and 23 fill the chip (2^20 and 2^25
  // lanes, 256 workgroups), batches of 2^(26 - d) blocks, 64 at most; d = 9 has
  // 2^11 lanes, 8 workgroups; a window of one counter has one lane.
  {
    const struct { unsigned d; uint64_t w; uint32_t nwg, batch; } chain[] = {
        {18, 1ull << 32, 256, 64}, {23, 1ull << 32, 256, 8}, {9, 1ull << 32, 8, 64}, {0, 1, 1, 64}};
    for (const auto& c : chain) {
      const PowChainPlan p = pow_chain_plan(c.d, c.w, 256, 2, 0);
      if (p.nwg != c.nwg || p.batch != c.batch) {
        ++failed;
        printf("chain d=%u window=%llu: nwg=%u batch=%u\n", c.d, (unsigned long long)c.w, p.nwg, p.batch);
      }
    }
    // Batch, planned lanes.  d = 13, window 2^32: the window cap leaves 2^38 /
    // 2^32 = 64 templates; 64 templates take one times 2^13 lanes (32
    // workgroups each: 64 x 32 exceeds the CUs at every step down), 2 templates
    // four times (128 each: 256 in all, not above the CUs).  d = 9, 1024
    // templates, window 2^16: 2^26 / 2^9 trials allow 2^17 templates, the tile
    // limit 2^14; lanes step down to 2^9, 2 workgroups each, 2^15 in all.
    const struct { unsigned d; uint64_t n, w; uint32_t nwg_t, tile; } batch[] = {
        {13, 64, 1ull << 32, 32, 64}, {13, 2, 1ull << 32, 128, 64}, {9, 1024, 1ull << 16, 2, 16384}};
    for (const auto& b : batch) {
      const PowBatchPlan p = pow_batch_plan(b.d, b.n, b.w, 256, -1, 0);
      if (p.nwg_t != b.nwg_t || p.tile != b.tile) {
        ++failed;
        printf("batch d=%u n=%llu window=%llu: nwg_t=%u tile=%u\n", b.d, (unsigned long long)b.n,
               (unsigned long long)b.w, p.nwg_t, p.tile);
      }
    }
  }
  printf("%ld plans, %ld failed\n", plans, failed);
  return failed ? 1 : 0;
}
