// The host plan of pow_pool_mark and pow_pool_prune (K12) on the CPU:
// pow_pool_prune_cap, pow_pool_prune_slots and pow_pool_prune_launches
// (csrc/pow_host.cpp), linked with pow_host.cpp alone and run under
// AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_pool_prune_host.py.
//   a. the capacity a prune leaves, for every kept count of a sweep and at the
//      seams, from several first capacities: a power of two that holds the
//      survivors and the first capacity, the lowest one, never past
//      POW_POOL_MAX_BLOCKS; the scratch the kernels take fits the arrays;
//   b. the table beside it: a power of two, slots >= 2 kept, and an add that
//      follows finds slots >= 2 size by the add's own rule;
//   c. prune, add, prune again: capacity and table shrink and grow;
//   d. the launch counts, by hand.
#include <algorithm>
#include <cstdint>
#include <cstdio>

#include "pow_host.h"

namespace {

long checks = 0, failed = 0;

#define CHECK(cond, ...)                \
  do {                                  \
    ++checks;                           \
    if (!(cond)) {                      \
      if (++failed <= 20) {             \
        printf("FAILED %s: ", #cond);   \
        printf(__VA_ARGS__);            \
        printf("\n");                   \
      }                                 \
    }                                   \
  } while (0)

bool pow2(uint32_t v) { return v && (v & (v - 1)) == 0; }

void check_cap(uint32_t kept, unsigned first_override) {
  const uint32_t first = pow_pool_live_first_cap(0, first_override);
  const uint32_t cap = pow_pool_prune_cap(kept, first);
  bool ok = pow2(cap) && cap >= kept && cap >= 1 && cap <= POW_POOL_MAX_BLOCKS;
  ok = ok && (cap >= first || cap == POW_POOL_MAX_BLOCKS);
  ok = ok && (cap == 1 || cap / 2 < std::max(kept, first));  // the lowest such power of two
  CHECK(ok, "cap %u for %u kept, first %u", cap, kept, first);
  for (unsigned lg : {0u, 1u, 5u, 21u}) {
    const uint32_t slots = pow_pool_prune_slots(cap, kept, lg);
    bool fine = pow2(slots) && slots >= 2 && slots >= 2ull * kept && slots <= (1u << 21);
    fine = fine && slots == pow_pool_live_slots(pow_pool_live_first_slots(cap, lg), kept);
    if (!lg) fine = fine && slots == std::max(2u, 2 * cap);  // what pow_pool_open takes at that capacity
    // the add that follows keeps its own promise from here
    const uint32_t after = pow_pool_live_slots(slots, std::min(kept + 1, POW_POOL_MAX_BLOCKS));
    fine = fine && after >= slots && after >= 2ull * std::min(kept + 1, POW_POOL_MAX_BLOCKS);
    CHECK(fine, "table %u for %u kept at cap %u, override %u", slots, kept, cap, lg);
  }
}

// The kernels' scratch in a pool of n blocks at capacity cap >= n: the marks (n
// bytes in whole words) in an array of cap words, one partial per 256 blocks in
// another, and the scan's 16 partials per lane of one workgroup hold them all.
void check_scratch(uint32_t n) {
  const uint32_t words = (n + 3) / 4, parts = (n + 255) / 256;
  CHECK(words <= n && parts <= n && parts <= 16 * 256 && (uint64_t)parts * 256 >= n && (uint64_t)words * 4 >= n,
        "scratch of %u blocks", n);
}

void caps() {
  for (unsigned fc : {0u, 1u, 2u, 3u, 100u, 1u << 20})
    for (uint32_t kept = 0; kept <= 5000; ++kept) check_cap(kept, fc);
  for (uint32_t e : {16u, 19u, 20u})
    for (int d = -2; d <= 2; ++d)
      if ((1ull << e) + d <= POW_POOL_MAX_BLOCKS)
        for (unsigned fc : {0u, 1u}) check_cap((uint32_t)((1ull << e) + d), fc);
  for (uint32_t n = 1; n <= 5000; ++n) check_scratch(n);
  for (uint32_t n : {(1u << 16) - 1, 1u << 16, (1u << 16) + 1, (1u << 20) - 1, 1u << 20}) check_scratch(n);
  CHECK(pow_pool_prune_cap(0, 64) == 64 && pow_pool_prune_cap(64, 64) == 64 && pow_pool_prune_cap(65, 64) == 128,
        "by hand at the shipped first capacity");
  CHECK(pow_pool_prune_cap(0, 1) == 1 && pow_pool_prune_cap(1, 1) == 1 && pow_pool_prune_cap(2, 1) == 2 &&
            pow_pool_prune_cap(3, 1) == 4 && pow_pool_prune_cap(0, 0) == 1,
        "by hand from one block");
  CHECK(pow_pool_prune_cap(POW_POOL_MAX_BLOCKS, 64) == POW_POOL_MAX_BLOCKS &&
            pow_pool_prune_cap((1u << 19) + 1, 64) == POW_POOL_MAX_BLOCKS && pow_pool_prune_cap(5, 1u << 21) == POW_POOL_MAX_BLOCKS,
        "never past the limit");
}

// A pool grown to `size` by adds, pruned to `kept`, grown again by `more`,
// pruned again: the capacity holds the pool and the table twice the pool at
// every step.
void cycle(unsigned first_override, unsigned slots_log2, uint32_t size, uint32_t kept, uint32_t more) {
  const uint32_t first = pow_pool_live_first_cap(0, first_override);
  uint32_t cap = first, slots = pow_pool_live_first_slots(cap, slots_log2);
  if (size > cap) cap = pow_pool_live_grow(cap, size);
  slots = pow_pool_live_slots(slots, size);
  const uint32_t cap0 = cap;
  cap = pow_pool_prune_cap(kept, first);
  slots = pow_pool_prune_slots(cap, kept, slots_log2);
  CHECK(cap <= cap0 && cap >= kept && slots >= 2ull * kept && pow2(slots), "pruned %u -> %u: cap %u -> %u, slots %u", size,
        kept, cap0, cap, slots);
  const uint32_t n = kept + more;
  if (n > cap) cap = pow_pool_live_grow(cap, n);
  slots = pow_pool_live_slots(slots, n);
  CHECK(cap >= n && pow2(cap) && slots >= 2ull * n && pow2(slots), "grown again to %u: cap %u, slots %u", n, cap, slots);
  const uint32_t again = n / 3;
  cap = pow_pool_prune_cap(again, first);
  slots = pow_pool_prune_slots(cap, again, slots_log2);
  CHECK(cap >= again && pow2(cap) && slots >= 2ull * again && pow2(slots), "pruned again to %u: cap %u, slots %u", again,
        cap, slots);
}

void cycles() {
  for (unsigned fc : {0u, 1u, 64u})
    for (unsigned lg : {0u, 1u})
      for (uint32_t size : {1u, 40u, 257u, 1025u, 65537u, 1u << 20})
        for (uint32_t kept : {0u, 1u, size / 3, size - 1})
          for (uint32_t more : {0u, 1u, 700u}) cycle(fc, lg, size, std::min(kept, size), std::min(more, POW_POOL_MAX_BLOCKS - kept));
}

void launches() {
  const struct { uint32_t size, kept; bool prune; uint32_t want; } by_hand[] = {
      {0, 0, false, 0},     {0, 0, true, 0},       {1, 1, false, 3},        {1, 0, true, 3},        {1, 1, true, 3},
      {2, 1, false, 4},     {2, 1, true, 7},       {40, 13, false, 9},      {40, 13, true, 12},     {40, 40, true, 9},
      {40, 0, true, 9},     {512, 1, true, 15},    {513, 512, true, 16},    {1025, 3, false, 14},   {65537, 300, true, 23},
      {1u << 20, 5, false, 23}, {1u << 20, 5, true, 26}, {(1u << 20) - 1, 1, true, 26}};
  for (const auto& c : by_hand)
    CHECK(pow_pool_prune_launches(c.size, c.kept, c.prune) == c.want, "size=%u kept=%u prune=%d: %u, stated %u", c.size,
          c.kept, (int)c.prune, pow_pool_prune_launches(c.size, c.kept, c.prune), c.want);
  for (uint32_t n = 1; n <= 5000; ++n) {
    const uint32_t r = pow_pool_rounds(n);
    CHECK((1ull << r) >= n && (r == 0 || (1ull << (r - 1)) < n), "rounds of %u", n);  // 2^r - 1 >= n - 1: the deepest walk
    CHECK(pow_pool_prune_launches(n, n / 2, false) == 3 + r, "mark of %u", n);
    CHECK(pow_pool_prune_launches(n, n / 2, true) == (n / 2 ? 6 : 3) + r, "prune of %u", n);
    CHECK(pow_pool_prune_launches(n, n, true) == 3 + r && pow_pool_prune_launches(n, 0, true) == 3 + r, "prune of %u, all or none", n);
  }
}

}  // namespace

int main() {
  caps();
  cycles();
  launches();
  printf("%ld checks, %ld failed\n", checks, failed);
  return failed ? 1 : 0;
}
