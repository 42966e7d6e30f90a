// The host plan of pow_index_blocks (K10) on the CPU: pow_pool_plan
// (csrc/pow_host.cpp), linked with pow_host.cpp alone and run
// under AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_pool_host.py.
//   a. the table's size, by hand for n = 1, 2, 3, 2^20 and as stated for every n
//      of a sweep, with and without the test library's override;
//   b. the round count, by hand for n = 1, 2, 3, 4, 5, 2^16 + 1 and as stated;
//   c. the buffer: every array inside it, none overlapping another, the
//      alignments the kernels rely on and the stated bytes per block;
//   d. the table's and the ranking's index arithmetic restated on small inputs:
//      linear probing with wrap-around meets an empty slot, and ceil(log2 n)
//      rounds of pointer jumping end every walk of a list of n nodes.
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

void sizes_by_hand() {
  const struct { uint32_t n, slots; } tables[] = {{1, 2}, {2, 4}, {3, 8}, {1u << 20, 1u << 21}};
  for (const auto& t : tables) {
    const PowPoolPlan p = pow_pool_plan(t.n, 0);
    CHECK(p.slots == t.slots, "n=%u: %u slots, stated %u", t.n, p.slots, t.slots);
  }
  const struct { uint32_t n, rounds; } rounds[] = {{1, 0}, {2, 1}, {3, 2}, {4, 2}, {5, 3}, {(1u << 16) + 1, 17},
                                                   {1u << 20, 20}};
  for (const auto& r : rounds) {
    const PowPoolPlan p = pow_pool_plan(r.n, 0);
    CHECK(p.rounds == r.rounds, "n=%u: %u rounds, stated %u", r.n, p.rounds, r.rounds);
  }
  // the forced minimum: the lowest power of two that leaves one slot empty
  const struct { uint32_t n, slots; } forced[] = {{1, 2}, {3, 4}, {40, 64}, {63, 64}, {64, 128}, {65, 128}, {127, 128},
                                                  {128, 256}, {1u << 20, 1u << 21}};
  for (const auto& f : forced) {
    const PowPoolPlan p = pow_pool_plan(f.n, 1);
    CHECK(p.slots == f.slots, "n=%u forced: %u slots, stated %u", f.n, p.slots, f.slots);
  }
  CHECK(pow_pool_plan(65, 0).slots == 256 && pow_pool_plan(64, 0).slots == 128, "the default at the wave tile");
  CHECK(pow_pool_plan(5, 10).slots == 1024 && pow_pool_plan(5, 99).slots == (1u << 21), "an override above the plan");
}

void check_plan(uint32_t n, unsigned lg) {
  const PowPoolPlan p = pow_pool_plan(n, lg);
  bool ok = pow2(p.slots) && p.slots >= n + 1u && p.slots <= (1u << 21);
  if (!lg) ok = ok && p.slots >= 2ull * n && (p.slots == 2 || p.slots / 2 < 2ull * n);
  ok = ok && (1ull << p.rounds) >= n && (p.rounds == 0 || (1ull << (p.rounds - 1)) < n);
  const uint32_t bytes = (n + 3) / 4;
  std::vector<std::pair<uint64_t, uint64_t>> a = {
      {p.ctl, 4}, {p.dig, 8ull * n}, {p.prev, 8ull * n}, {p.index, n}, {p.parent, n}, {p.next[0], n}, {p.next[1], n},
      {p.depth[0], n}, {p.depth[1], n}, {p.bad[0], n}, {p.bad[1], n}, {p.status, bytes}, {p.kind, bytes},
      {p.table, p.slots}};
  uint64_t sum = 0;
  for (const auto& x : a) {
    ok = ok && x.first + x.second <= p.words;
    sum += x.second;
  }
  std::sort(a.begin(), a.end());
  for (size_t k = 0; k + 1 < a.size(); ++k) ok = ok && a[k].first + a[k].second <= a[k + 1].first;
  ok = ok && sum == p.words && p.words == 4 + 24ull * n + 2ull * bytes + p.slots && p.words < (1ull << 32);
  ok = ok && p.ctl % 2 == 0 && p.dig % 4 == 0 && p.prev % 4 == 0;  // 8 bytes for the 64-bit key, 16 for the vectors
  ok = ok && p.words * 4 < 16 + 98ull * n + 8 + 4ull * p.slots;     // 98 bytes per block, status and kind rounded up
  CHECK(ok, "plan n=%u slots_log2=%u: slots=%u rounds=%u words=%llu", n, lg, p.slots, p.rounds, (unsigned long long)p.words);
}

void plan_sweep() {
  for (uint32_t n = 1; n <= 5000; ++n)
    for (unsigned lg : {0u, 1u, 7u, 21u, 40u}) check_plan(n, lg);
  for (uint32_t e = 12; e <= 20; ++e)
    for (int d = -2; d <= 2; ++d) {
      const uint64_t n = (1ull << e) + d;
      if (n <= (1u << 20))
        for (unsigned lg : {0u, 1u, 16u, 21u}) check_plan((uint32_t)n, lg);
    }
  const PowPoolPlan big = pow_pool_plan(1u << 20, 0);
  CHECK(big.words * 4 == 16 + (98ull << 20) + (4ull << 21), "2^20 blocks: %llu bytes", (unsigned long long)big.words * 4);
}

// K10b's and K10c's probe, restated: every key starts at the same slot, the
// worst a table can meet; all find a slot within the table's size, wrapping at
// its end, and a lookup ends at the key or at an empty slot.
void probe_model() {
  for (uint32_t n : {1u, 2u, 3u, 40u, 63u, 64u, 65u, 127u}) {
    const PowPoolPlan p = pow_pool_plan(n, 1);
    const uint32_t mask = p.slots - 1;
    std::vector<uint32_t> table(p.slots, ~0u);
    bool ok = true;
    for (uint32_t i = 0; i < n; ++i) {
      uint32_t slot = (p.slots - 2u) & mask, probe = 0;  // two in front of the end: the third key wraps
      for (; probe <= mask; ++probe) {
        if (table[slot] == ~0u) {
          table[slot] = i;
          break;
        }
        slot = (slot + 1) & mask;
      }
      ok = ok && probe <= mask;
    }
    for (uint32_t i = 0; i <= n; ++i) {  // key n is not in the table
      uint32_t slot = (p.slots - 2u) & mask, found = ~0u;
      for (uint32_t probe = 0; probe <= mask; ++probe) {
        if (table[slot] == ~0u || table[slot] == i) {
          found = table[slot];
          break;
        }
        slot = (slot + 1) & mask;
      }
      ok = ok && found == (i < n ? i : ~0u);
    }
    CHECK(ok, "probes at n=%u, %u slots", n, p.slots);
  }
}

// K10d's round and K10e's rule, restated, on one list of n nodes laid out in
// a scrambled order: after the plan's rounds every walk has ended and the
// depths are exact; one round fewer leaves the deepest walk open when n > 1.
void rank_model() {
  for (uint32_t n : {1u, 2u, 3u, 4u, 5u, 8u, 9u, 1000u, 1024u, 1025u}) {
    const uint32_t rounds = pow_pool_plan(n, 0).rounds;
    std::vector<uint32_t> order(n), want(n);
    for (uint32_t k = 0; k < n; ++k) order[k] = (uint32_t)((k * 7919ull + 13) % n);  // 7919 is prime: a permutation
    std::vector<uint32_t> next(n), depth(n, 1), nn(n), dd(n);
    for (uint32_t k = 0; k < n; ++k) {  // order[k]'s parent is order[k - 1]; order[0] is the root
      next[order[k]] = k ? order[k - 1] : 0xFFFFFFFFu;
      want[order[k]] = k + 1;
    }
    bool open_before = false;
    for (uint32_t r = 0; r < rounds; ++r) {
      if (r + 1 == rounds) open_before = std::any_of(next.begin(), next.end(), [&](uint32_t v) { return v < n; });
      for (uint32_t i = 0; i < n; ++i) {
        uint32_t nx = next[i], d = depth[i];
        if (nx < n) {
          d += depth[nx];
          nx = next[nx];
        }
        nn[i] = nx;
        dd[i] = d;
      }
      next.swap(nn);
      depth.swap(dd);
    }
    const bool ended = std::none_of(next.begin(), next.end(), [&](uint32_t v) { return v < n; });
    CHECK(ended && depth == want && (rounds == 0 || open_before), "ranking a list of %u in %u rounds", n, rounds);
  }
}

}  // namespace

int main() {
  sizes_by_hand();
  plan_sweep();
  probe_model();
  rank_model();
  printf("%ld checks, %ld failed\n", checks, failed);
  return failed ? 1 : 0;
}
