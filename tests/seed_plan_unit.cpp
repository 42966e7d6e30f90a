// The host side of pow_find_seed (K9) on the CPU: pow_seed_plan, pow_seed_pack
// and the arithmetic the kernel copies (csrc/pow_host.cpp), linked with
// pow_host.cpp alone and run under AddressSanitizer + UndefinedBehaviorSanitizer
// by tests/test_seed_host.py.  Four parts:
//   a. the plan over a grid of seeds, windows, chip sizes and overrides: what
//      pow_host.h promises, and that its tiles and slices cover every (seed,
//      trial) of the request exactly once;
//   b. pow_seed_pack: the round trip through pow_nonce_from_counter, and every
//      byte outside the alphabet refused;
//   c. pow_seed.hip's seeding restated (the circular window of 31 words)
//      against pow_rand_seed;
//   d. pow_seed.hip's walk restated (whole iterations of 31 trials, the bound
//      applied where a trial is recorded, the hop and the step polynomial):
//      every trial of the slice is recorded exactly once, with the nonce of
//      pow_rand_nonces, and none outside it.  A model, not the kernel: it pins
//      the host-made polynomials and the index arithmetic.
#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
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

const uint32_t SEEDS[] = {0u, 1u, 2u, 0x7FFFFFFFu, 0x80000000u, 0x80000001u, 0xFFFFFFFEu, 0xFFFFFFFFu, 1700000003u};

bool run_ok(uint32_t run) {
  const uint32_t j = run / 31u;
  return run % 31u == 0 && j >= 1 && j <= 32 && (j & (j - 1)) == 0;
}

// ---- a ----
void plan_sweep() {
  const uint32_t seeds[] = {1, 2, 3, 16, 17, 255, 256, 257, 4096, 65536, 65537, 1u << 20};
  const uint64_t counts[] = {1, 31, 32, 7935, 7936, 7937, 1ull << 16, 1ull << 20, (1ull << 26) - 1, 1ull << 26,
                             (1ull << 26) + 1, 1ull << 30, 1ull << 32};
  const uint32_t cus[] = {0, 1, 8, 104, 256, 304, 1024};
  const unsigned runs[] = {0, 1, 30, 31, 32, 61, 62, 63, 124, 991, 992, 993, 1024, UINT_MAX};
  const unsigned wgs[] = {0, 1, 2, 3, 255, 256, 257, UINT_MAX};
  const unsigned launches[] = {0, 1, 5, 13, 26, 27, 30, 31, 99};
  for (uint32_t ns : seeds)
    for (uint64_t count : counts)
      for (uint32_t cu : cus)
        for (unsigned ro : runs)
          for (unsigned wo : wgs)
            for (unsigned lg : launches) {
              const PowSeedPlan p = pow_seed_plan(ns, count, cu, ro, wo, lg);
              const uint64_t cap = 1ull << std::min(lg, 30u);
              bool ok = p.nwg >= 1 && p.nwg <= POW_RAND_MAX_WG;
              ok = ok && run_ok(p.run) && p.run <= POW_RAND_MAX_RUN;
              ok = ok && p.tile >= 1 && p.tile <= ns && (uint64_t)p.tile * p.nwg <= (1u << 16);
              ok = ok && p.slice >= 1 && p.slice <= (1ull << 26) && p.slice <= count;
              const uint64_t pass = (uint64_t)p.nwg * 256u * p.run;
              ok = ok && pass <= (1ull << 26) && pass + p.slice <= (1ull << 27);  // the kernel's rel, 32 bits, after a hop
              ok = ok && ((uint64_t)p.tile * p.slice <= cap || p.tile == 1);       // a launch's pairs (one seed: the slice alone)
              ok = ok && p.slice <= std::max<uint64_t>(cap, 1);
              if (wo) ok = ok && p.nwg == std::min(wo, POW_RAND_MAX_WG);
              if (ro) {
                uint32_t r = 31;
                while (r < 992 && 2ull * r <= ro) r *= 2;
                ok = ok && p.run == r;
              } else {
                ok = ok && (p.run == 31 || pass <= p.slice);  // one pass lies inside the slice
              }
              // exact cover: the tiles cut [0, ns) and the slices [0, count), each into consecutive pieces
              // (pow_find_seed's two loops), so the pairs of all launches sum to the request's.  Walked
              // launch by launch while there are few, by whole rows and columns above that.
              const uint64_t tiles = (ns + p.tile - 1) / p.tile, slices = (count + p.slice - 1) / p.slice;
              unsigned __int128 sum = 0;
              if (tiles * slices <= 512) {
                for (uint64_t b = 0; b < ns; b += p.tile)
                  for (uint64_t off = 0; off < count; off += p.slice) {
                    const uint64_t pairs = std::min<uint64_t>(p.tile, ns - b) * std::min<uint64_t>(p.slice, count - off);
                    ok = ok && pairs <= cap;
                    sum += pairs;
                  }
              } else {
                const uint64_t last_tile = ns - (tiles - 1) * p.tile, last_slice = count - (slices - 1) * p.slice;
                ok = ok && last_tile >= 1 && last_tile <= p.tile && last_slice >= 1 && last_slice <= p.slice;
                sum = (unsigned __int128)((tiles - 1) * p.tile + last_tile) * ((slices - 1) * p.slice + last_slice);
              }
              ok = ok && sum == (unsigned __int128)ns * count;
              CHECK(ok, "plan seeds=%u count=%llu cu=%u run_override=%u wg_override=%u launch_log2=%u: tile=%u nwg=%u run=%u slice=%llu",
                    ns, (unsigned long long)count, cu, ro, wo, lg, p.tile, p.nwg, p.run, (unsigned long long)p.slice);
            }
  // The shipped shapes on 256 CUs by hand.  One seed, 2^32 trials: slices of
  // 2^26 with table B's 256 workgroups and T = 992 (256 x 256 x 992 < 2^26).
  // 4,096 seeds, 2^20 trials: 2^30 / 2^20 = 1,024 seeds per launch, 2 workgroups
  // each, T = 992 (2 x 256 x 992 <= 2^20).  One seed, one trial: one lane's worth.
  const struct { uint32_t ns; uint64_t n; uint32_t tile, nwg, run; uint64_t slice; } shapes[] = {
      {1, 1ull << 32, 1, 256, 992, 1ull << 26}, {4096, 1ull << 20, 1024, 2, 992, 1ull << 20}, {1, 1, 1, 1, 31, 1},
      {1u << 20, 1ull << 32, 16, 128, 992, 1ull << 26}};
  for (const auto& s : shapes) {
    const PowSeedPlan p = pow_seed_plan(s.ns, s.n, 256, 0, 0, 30);
    CHECK(p.tile == s.tile && p.nwg == s.nwg && p.run == s.run && p.slice == s.slice,
          "shipped seeds=%u n=%llu: tile=%u nwg=%u run=%u slice=%llu", s.ns, (unsigned long long)s.n, p.tile, p.nwg, p.run,
          (unsigned long long)p.slice);
  }
}

// ---- b ----
void pack() {
  uint32_t lcg = 99u;
  const uint64_t limit = 13537086546263552ull;  // 62^9
  for (int k = 0; k < 20000; ++k) {
    uint64_t ctr;
    if (k < 4) {
      const uint64_t corner[4] = {0, 1, limit - 1, 62ull * 62 * 62 * 62};
      ctr = corner[k];
    } else {
      lcg = lcg * 1664525u + 1013904223u;
      ctr = (uint64_t)lcg << 22;
      lcg = lcg * 1664525u + 1013904223u;
      ctr = (ctr ^ lcg) % limit;
    }
    char nonce[POW_NONCE_SIZE];
    uint32_t w[2] = {~0u, ~0u};
    const bool ok = pow_nonce_from_counter(ctr, nonce) == POW_OK && pow_seed_pack(nonce, w);
    uint64_t back = 0;
    for (int i = 4; i >= 0; --i) back = back * 62 + ((w[0] >> (6 * i)) & 63u);
    for (int i = 3; i >= 0; --i) back = back * 62 + ((w[1] >> (6 * i)) & 63u);
    CHECK(ok && back == ctr && w[0] < (1u << 30) && w[1] < (1u << 24), "pack ctr=%llu: \"%.9s\" -> %08x %08x -> %llu",
          (unsigned long long)ctr, nonce, w[0], w[1], (unsigned long long)back);
  }
  for (int c = 0; c < 256; ++c)
    for (int at = 0; at < 9; ++at) {
      char nonce[POW_NONCE_SIZE] = "aZ09bY18c";
      nonce[at] = (char)c;
      uint32_t w[2] = {0xAAAAAAAAu, 0xAAAAAAAAu};
      const bool alnum = (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || (c >= '0' && c <= '9');
      const bool got = pow_seed_pack(nonce, w);
      CHECK(got == alnum && (got || (w[0] == 0xAAAAAAAAu && w[1] == 0xAAAAAAAAu)), "pack byte %d at %d", c, at);
    }
  // byte 9 is not read
  char nonce[POW_NONCE_SIZE] = "abcdefghi";
  uint32_t a[2], b[2];
  nonce[9] = '\xFF';
  CHECK(pow_seed_pack(nonce, a), "byte 9");
  nonce[9] = 0;
  CHECK(pow_seed_pack(nonce, b) && a[0] == b[0] && a[1] == b[1], "byte 9");
}

// ---- c ----
void seed_state(uint32_t seed, uint32_t x[31]) {  // pow_seed.hip's
  uint32_t r[31];
  r[0] = seed ? seed : 1u;
  for (uint32_t i = 1; i < 31; ++i) {
    const int32_t w = (int32_t)r[i - 1];
    const int32_t hi = w / 127773, lo = w - hi * 127773;
    long long v = 16807ll * lo - 2836ll * hi;
    if (v < 0) v += 2147483647;
    r[i] = (uint32_t)v;
  }
  for (uint32_t i = 34; i < 344; ++i) r[i % 31] += r[(i - 3) % 31];
  for (uint32_t j = 0; j < 31; ++j) x[j] = r[(j + 3) % 31];
}

void seeding() {
  for (uint32_t seed : SEEDS) {
    uint32_t want[31], got[31];
    pow_rand_seed(seed, want);
    seed_state(seed, got);
    CHECK(memcmp(want, got, sizeof want) == 0, "seeding of %u", seed);
  }
  uint32_t lcg = 7u;
  for (int k = 0; k < 2000; ++k) {
    lcg = lcg * 1664525u + 1013904223u;
    uint32_t want[31], got[31];
    pow_rand_seed(lcg, want);
    seed_state(lcg, got);
    CHECK(memcmp(want, got, sizeof want) == 0, "seeding of %u", lcg);
  }
}

// ---- d ----
void lane_walk() {
  const uint32_t seed = 0x80000001u;
  const uint64_t start = (1ull << 40) + 7;
  std::vector<uint32_t> tab(POW_RAND_TAB_WORDS);
  const uint32_t* const A = tab.data();
  const uint32_t* const B = tab.data() + POW_RAND_WORDS * 256u;
  uint32_t launch_state[31], jump[31];
  seed_state(seed, launch_state);
  pow_rand_power(9ull * start, jump);
  pow_rand_apply(jump, launch_state, launch_state);
  const uint32_t most = 2u * 2u * 256u * 62u + 40u;
  std::vector<char> want((size_t)most * POW_NONCE_SIZE);
  if (pow_rand_nonces(seed, start, most, want.data()) != POW_OK) {
    CHECK(false, "pow_rand_nonces: %s", pow_last_error());
    return;
  }
  const uint32_t Ts[] = {31, 62};
  for (uint32_t nwg = 1; nwg <= 2; ++nwg)
    for (uint32_t T : Ts) {
      const uint32_t G = nwg * 256u;
      pow_rand_tables(T, tab.data());
      uint32_t step[31];
      pow_rand_power(9ull * T * ((uint64_t)G - 1u), step);
      const uint32_t counts[] = {1, 30, 31, 32, T + 1, G * T - 1, G * T, G * T + 1, 2 * G * T + 33};
      for (uint32_t count : counts) {
        std::vector<uint8_t> seen(count, 0);
        long wrong_nonce = 0;
        for (uint32_t part = 0; part < nwg; ++part)
          for (uint32_t tid = 0; tid < 256u; ++tid) {
            uint32_t x[31], col[31];
            pow_rand_apply(B + part * 31u, launch_state, x);
            for (uint32_t i = 0; i < 31u; ++i) col[i] = A[i * 256u + tid];
            pow_rand_apply(col, x, x);
            const uint32_t iters = T / 31u, hop_by = nwg * 256u * T - T;
            uint32_t rel = (part * 256u + tid) * T;
            while (rel < count) {
              for (uint32_t it = 0; it < iters; ++it) {
                for (uint32_t t = 0; t < 31u; ++t) {  // the circular form of the kernel: the head is (9 t + i) % 31
                  for (uint32_t i = 0; i < 9u; ++i) {
                    const uint32_t h = (9u * t + i) % 31u;
                    x[h] += x[(h + 28u) % 31u];
                  }
                  char nonce[POW_NONCE_SIZE];
                  for (uint32_t i = 0; i < 9u; ++i) {
                    const uint32_t d = (x[(9u * t + i) % 31u] >> 1) % 62u;
                    nonce[i] = d < 26 ? (char)('a' + d) : d < 52 ? (char)('A' + d - 26) : (char)('0' + d - 52);
                  }
                  nonce[9] = 0;
                  if (rel + t < count) {  // the bound where a trial is recorded
                    if (seen[rel + t] < 255) ++seen[rel + t];
                    if (memcmp(nonce, want.data() + (size_t)(rel + t) * POW_NONCE_SIZE, POW_NONCE_SIZE) != 0) ++wrong_nonce;
                  }
                }
                rel += 31u;
              }
              rel += hop_by;
              if (rel < count) pow_rand_apply(step, x, x);  // the head is back at 0: x is in the host's order
            }
          }
        const long once = std::count(seen.begin(), seen.end(), 1);
        CHECK(once == (long)count, "walk nwg=%u T=%u count=%u: %ld trials recorded exactly once", nwg, T, count, once);
        CHECK(wrong_nonce == 0, "walk nwg=%u T=%u count=%u: %ld trials drew another nonce than pow_rand_nonces", nwg, T, count,
              wrong_nonce);
      }
    }
}

}  // namespace

int main() {
  plan_sweep();
  pack();
  seeding();
  lane_walk();
  printf("%ld checks, %ld failed\n", checks, failed);
  return failed ? 1 : 0;
}
