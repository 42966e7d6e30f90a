// The plan of pow_mine_race's fused path (pow_race_plan, csrc/pow_host.cpp) on
// the CPU: linked with pow_host.cpp alone and run under AddressSanitizer +
// UndefinedBehaviorSanitizer by tests/test_race_host.py.  Over every
// difficulty, rival count, chip size and window of the lists below it checks
// what pow_host.h promises and pow_mine_race relies on for its slots, its
// batch buffers and its watchdog.
#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "pow_host.h"

int main() {
  const uint32_t rivals[] = {1, 2, 3, 64, 255, 256};
  const uint32_t cus[] = {1, 32, 256};
  const uint64_t windows[] = {1, 2, 255, 256, 257, 700, 1ull << 12, 1ull << 16, (1ull << 16) + 1, 1ull << 24, 1ull << 30,
                              (1ull << 32) - 1, 1ull << 32};
  const unsigned lanes[] = {0, 2, 7, 8};
  const unsigned overrides[] = {0, 1, 2, 64};
  long plans = 0, failed = 0;
  for (unsigned d = 0; d <= 32; ++d)
    for (uint32_t R : rivals)
      for (uint32_t cu : cus)
        for (uint64_t w : windows)
          for (unsigned ll : lanes)
            for (unsigned ov : overrides) {
              PowRacePlan p{0xFFFFFFFFu, 0xFFFFFFFFu};
              pow_race_plan(d, R, w, cu, ll, ov, &p);
              ++plans;
              bool ok = p.nwg_r >= 1;
              ok = ok && (uint64_t)p.nwg_r * R <= std::max<uint64_t>(R, cu);
              ok = ok && p.batch >= 1 && p.batch <= 64;
              ok = ok && (p.batch == 1 || (uint64_t)p.batch * R * w <= (1ull << 38));
              // a rival has no more lanes than its window has counters, but for the one workgroup it always gets
              ok = ok && (p.nwg_r == 1 || (uint64_t)(p.nwg_r - 1) * 256 < w);
              if (ov) ok = ok && p.batch <= ov;
              if (!ok) {
                ++failed;
                if (failed <= 20)
                  printf("d=%u R=%u cu=%u window=%llu lanes_log2=%u override=%u: nwg_r=%u batch=%u\n", d, R, cu,
                         (unsigned long long)w, ll, ov, p.nwg_r, p.batch);
              }
            }
  // the shipped shape: three rivals at d = 18 on 256 CUs get lanes for four times 2^18 trials
  {
    PowRacePlan p{};
    pow_race_plan(18, 3, 1ull << 32, 256, 2, 0, &p);
    if (p.nwg_r != 85 || p.batch != 21) {
      ++failed;
      printf("d=18 R=3: nwg_r=%u batch=%u\n", p.nwg_r, p.batch);
    }
    pow_race_plan(9, 64, 1ull << 16, 256, 2, 0, &p);  // 2^11 lanes over 64 rivals: one workgroup each
    if (p.nwg_r != 1 || p.batch != 64) {
      ++failed;
      printf("d=9 R=64: nwg_r=%u batch=%u\n", p.nwg_r, p.batch);
    }
  }
  printf("%ld plans, %ld failed\n", plans, failed);
  return failed ? 1 : 0;
}
