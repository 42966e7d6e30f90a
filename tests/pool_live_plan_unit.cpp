// The host plan of pow_pool (K11) on the CPU: pow_pool_live_plan and its
// companions (csrc/pow_host.cpp), linked with pow_host.cpp alone and run under
// AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_pool_stream_host.py.
//   a. the arrays at every capacity of a sweep and at the seams 2^16 and 2^20:
//      each inside the buffer, none overlapping another, the alignments the
//      kernels rely on, 98 bytes per block;
//   b. pools fed in steps of several sizes from several first capacities and
//      first tables: slots >= 2 x size after every add, a power of two, rebuilt
//      only when it has to be; the capacity grows by doubling, holds the pool
//      and never passes POW_POOL_MAX_BLOCKS;
//   c. the launch counts, by hand and against pow_index_blocks' plan for the
//      batch alone.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

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

void check_arrays(uint32_t cap) {
  const PowPoolLivePlan p = pow_pool_live_plan(cap);
  const uint64_t n = cap, bytes = (n + 3) / 4;
  std::vector<std::pair<uint64_t, uint64_t>> a = {
      {p.ctl, POW_POOL_LIVE_CTL_WORDS}, {p.dig, 8 * n}, {p.prev, 8 * n}, {p.index, n}, {p.parent, n},
      {p.next[0], n}, {p.next[1], n}, {p.depth[0], n}, {p.depth[1], n}, {p.bad[0], n}, {p.bad[1], n},
      {p.status, bytes}, {p.kind, bytes}};
  bool ok = p.cap == cap;
  for (const auto& x : a) ok = ok && x.first + x.second <= p.words;
  std::sort(a.begin(), a.end());
  for (size_t k = 0; k + 1 < a.size(); ++k) ok = ok && a[k].first + a[k].second <= a[k + 1].first;
  ok = ok && p.words == 8 + 24 * n + 2 * bytes && p.words < (1ull << 32);
  ok = ok && p.ctl % 2 == 0 && p.dig % 4 == 0 && p.prev % 4 == 0;  // 8 bytes for the 64-bit key, 16 for the vectors
  ok = ok && p.words * 4 < 32 + 98 * n + 8;                        // 98 bytes per block, status and kind rounded up
  CHECK(ok, "arrays at cap=%u: words=%llu", cap, (unsigned long long)p.words);
}

void arrays_sweep() {
  for (uint32_t cap = 1; cap <= 4000; ++cap) check_arrays(cap);
  for (uint32_t e : {16u, 20u})
    for (int d = -2; d <= 2; ++d)
      if ((1ull << e) + d <= POW_POOL_MAX_BLOCKS) check_arrays((uint32_t)((1ull << e) + d));
}

// One pool fed in steps of `step` blocks up to `upto`, as pow_pool_open and
// pow_pool_add use the plan.
void feed(size_t reserve, unsigned first_cap, unsigned slots_log2, uint32_t step, uint32_t upto) {
  uint32_t cap = pow_pool_live_first_cap(reserve, first_cap);
  uint32_t slots = pow_pool_live_first_slots(cap, slots_log2);
  CHECK(cap >= 1 && cap <= POW_POOL_MAX_BLOCKS && cap == (reserve ? reserve : first_cap ? first_cap : 64u),
        "first cap %u of reserve %zu, override %u", cap, reserve, first_cap);
  CHECK(pow2(slots) && slots >= 2 && slots <= (1u << 21) && (slots_log2 ? slots == 1u << slots_log2 : slots >= 2 * cap),
        "first table %u of cap %u, override %u", slots, cap, slots_log2);
  uint32_t size = 0, grown = 0;
  while (size < upto) {
    const uint32_t m = std::min(step, upto - size), n = size + m;
    if (n > cap) {
      const uint32_t to = pow_pool_live_grow(cap, n);
      bool ok = to >= n && to <= POW_POOL_MAX_BLOCKS && to > cap;
      uint64_t c = cap;  // by doubling: cap x 2^k with the least k that holds n, or the limit
      while (c < n) c *= 2;
      ok = ok && to == std::min<uint64_t>(c, POW_POOL_MAX_BLOCKS) && (c / 2 < n);
      CHECK(ok, "growth %u -> %u for %u blocks", cap, to, n);
      cap = to;
      ++grown;
    }
    const uint32_t s = pow_pool_live_slots(slots, n);
    bool ok = pow2(s) && s >= 2ull * n && s <= (1u << 21) && s >= slots;
    if (n <= slots / 2) ok = ok && s == slots;   // no rebuild that is not needed
    else ok = ok && s / 2 < 2ull * n;            // a rebuild takes the lowest power of two
    CHECK(ok, "table %u -> %u for %u blocks", slots, s, n);
    slots = s;
    size = n;
  }
  if (!reserve && !first_cap && upto >= 1024 && step <= 512) CHECK(grown >= 2, "reserve 0: grown %u times by %u blocks", grown, upto);
}

void feeds() {
  for (uint32_t step : {1u, 2u, 5u, 50u, 130u})
    for (unsigned lg : {0u, 1u, 5u, 21u})
      for (unsigned fc : {0u, 1u, 2u, 100u}) feed(0, fc, lg, step, 3000);
  for (size_t reserve : {1u, 513u, 4096u}) feed(reserve, 0, 0, 50, 5000);
  for (uint32_t upto : {(1u << 16) - 1, 1u << 16, (1u << 16) + 1, (1u << 20) - 1, 1u << 20}) {
    feed(0, 0, 0, 65536, upto);
    feed(0, 0, 1, 99991, upto);
    feed(upto, 0, 0, upto, upto);
  }
  CHECK(pow_pool_live_grow(1u << 19, (1u << 20)) == (1u << 20) && pow_pool_live_grow(700000, 700001) == (1u << 20),
        "growth stops at the limit");
  CHECK(pow_pool_live_first_cap((size_t)1 << 40, 0) == POW_POOL_MAX_BLOCKS, "a reserve past the limit");
}

void launches() {
  const struct { uint32_t m, size; bool rerank; uint32_t want; } by_hand[] = {
      {1, 1, false, 4},        {1, 1000, false, 4},   {2, 2, false, 5},          {5, 36, false, 7},
      {1u << 16, 1u << 16, false, 20}, {(1u << 16) + 1, (1u << 16) + 1, false, 22},
      {1, 2, true, 4 + 3 + 1}, {1, 40, true, 4 + 3 + 6}, {1, (1u << 16) + 1, true, 4 + 3 + 17},
      {1u << 20, 1u << 20, true, 16 + 3 + 20 + 3 + 20}};
  for (const auto& c : by_hand)
    CHECK(pow_pool_live_launches(c.m, c.size, c.rerank) == c.want, "m=%u size=%u rerank=%d: %u, stated %u", c.m, c.size,
          (int)c.rerank, pow_pool_live_launches(c.m, c.size, c.rerank), c.want);
  for (uint32_t m = 1; m <= 5000; ++m) {  // what pow_index_blocks takes on the m blocks alone
    const uint32_t alone = 1 + 3 + pow_pool_plan(m, 0).rounds;
    CHECK(pow_pool_live_launches(m, m + 17, false) == alone && pow_pool_rounds(m) == pow_pool_plan(m, 0).rounds,
          "m=%u", m);
    CHECK(pow_pool_live_launches(m, m + 17, true) == alone + 3 + pow_pool_plan(m + 17, 0).rounds, "m=%u re-ranked", m);
  }
  CHECK(pow_pool_rounds(0) == 0 && pow_pool_rounds(1) == 0 && pow_pool_rounds(1u << 20) == 20, "rounds");
}

}  // namespace

int main() {
  arrays_sweep();
  feeds();
  launches();
  printf("%ld checks, %ld failed\n", checks, failed);
  return failed ? 1 : 0;
}
