// The host side of pow_mine_rand (K8) on the CPU: pow_rand_plan, pow_rand_tables
// and the polynomials the kernel consumes (csrc/pow_host.cpp), linked with
// pow_host.cpp alone and run under AddressSanitizer + UndefinedBehaviorSanitizer
// by tests/test_rand_host.py.  Four parts:
//   a. the plan over every difficulty, window, chip size and override of the
//      lists below: what pow_host.h promises, what the kernel's 32-bit trial
//      index needs, and that the planned run is the least that covers;
//   b. the tables: the seeded state moved by B[w] and then by A[.][l] stands at
//      trial start + T (256 w + l);
//   c. the lane walk of pow_rand.hip restated (rel, in_run, hop_by, the step
//      polynomial): every trial of the launch is visited exactly once, with the
//      nonce of pow_rand_nonces.  A model, not the kernel: it pins the
//      host-made polynomials and the arithmetic the kernel copies;
//   d. what pow_mine_rand and pow_find_seed share: pow_rand_jumps against
//      pow_rand_power, and digit_of against the alphabet, every byte value.
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

const uint32_t SEEDS[] = {0u, 1u, 0x80000000u, 0xFFFFFFFFu, 1700000003u};
const uint64_t STARTS[] = {0, 1234577, (1ull << 40) + 123};

uint32_t lcg_state = 12345u;
uint32_t lcg() {  // the tests' own numbers: no rand(), no process-global state of libc
  lcg_state = lcg_state * 1664525u + 1013904223u;
  return lcg_state >> 8;
}

// The state of srand(seed) at trial `trial`.
void state_at(uint32_t seed, uint64_t trial, uint32_t x[POW_RAND_WORDS]) {
  uint32_t jump[POW_RAND_WORDS];
  pow_rand_seed(seed, x);
  pow_rand_power(9ull * trial, jump);
  pow_rand_apply(jump, x, x);
}

// ---- a ----
void plan_sweep() {
  const uint64_t counts[] = {1, 2, 255, 256, 257, 1000, 1ull << 16, 1ull << 20, 1ull << 26, (1ull << 26) + 1, 1ull << 32};
  const uint32_t cus[] = {0, 1, 8, 104, 256, 304, 1024};
  const int lanes[] = {-1, 0, 8, 9, 10, 16, 40};
  const unsigned runs[] = {0, 1, 2, 3, 4, 63, 64, 1000, 1024, 1025, UINT_MAX};
  const unsigned launches[] = {0, 1, 10, 26, 27, 99};
  const unsigned diffs[] = {0,  1,  2,  3,  4,  5,  6,  7,  8,  9,  10, 11, 12, 13, 14, 15, 16, 17, 18,
                            19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 64, UINT_MAX};
  for (unsigned diff : diffs)
    for (uint64_t count : counts)
      for (uint32_t cu : cus)
        for (int ll : lanes)
          for (unsigned ov : runs)
            for (unsigned lg : launches) {
              const PowRandPlan p = pow_rand_plan(diff, count, cu, ll, ov, lg);
              const unsigned d = std::min(diff, 32u);
              const uint64_t n = std::min(p.launch, count);
              const uint64_t pass = (uint64_t)p.nwg * 256u * p.run;
              const uint64_t want = std::min<uint64_t>(4ull << d, n);
              bool ok = p.launch >= 1 && p.launch <= (1ull << 26);
              ok = ok && p.launch == 1ull << std::min(lg, 26u);
              ok = ok && p.nwg >= 1 && p.nwg <= std::min(std::max(1u, cu), POW_RAND_MAX_WG);
              ok = ok && (uint64_t)(p.nwg - 1) * 256 < n;  // no workgroup starts past the launch
              ok = ok && p.run >= 1 && p.run <= POW_RAND_MAX_RUN && (p.run & (p.run - 1)) == 0;
              ok = ok && pass <= (1ull << 26);
              ok = ok && pass + n <= (1ull << 27);  // the kernel's rel, 32 bits, after a hop
              if (ov) {
                uint32_t r = 1;
                while (2ull * r <= std::min<uint64_t>(ov, POW_RAND_MAX_RUN)) r *= 2;
                ok = ok && p.run == r;
              } else {
                ok = ok && (p.run == 1 || pass / 2 < want);                  // minimal
                ok = ok && (p.run == POW_RAND_MAX_RUN || pass >= want);      // sufficient
              }
              CHECK(ok, "plan d=%u count=%llu cu=%u lanes_log2=%d run_override=%u launch_log2=%u: launch=%llu nwg=%u run=%u",
                    diff, (unsigned long long)count, cu, ll, ov, lg, (unsigned long long)p.launch, p.nwg, p.run);
            }
  // The shipped shapes on 256 CUs by hand.  d = 9, 2^32 trials: 2^11 lanes, 8
  // workgroups, one trial each.  d = 17: 4 x 2^17 = 2^19 trials over 2^16
  // lanes, T = 8.  d = 32: the launch's 2^26 trials, T = 1,024.
  const struct { unsigned d; uint64_t n; uint32_t nwg, run; } shapes[] = {
      {9, 1ull << 32, 8, 1}, {17, 1ull << 32, 256, 8}, {32, 1ull << 32, 256, 1024}, {17, 1, 1, 1}};
  for (const auto& s : shapes) {
    const PowRandPlan p = pow_rand_plan(s.d, s.n, 256, -1, 0, 26);
    CHECK(p.launch == (1ull << 26) && p.nwg == s.nwg && p.run == s.run, "shipped d=%u n=%llu: nwg=%u run=%u", s.d,
          (unsigned long long)s.n, p.nwg, p.run);
  }
}

// ---- b ----
void tables() {
  std::vector<uint32_t> tab(POW_RAND_TAB_WORDS);
  const uint32_t* const A = tab.data();
  const uint32_t* const B = tab.data() + POW_RAND_WORDS * 256u;
  const uint32_t Ts[] = {1, 2, 64, 1024};
  for (uint32_t T : Ts) {
    pow_rand_tables(T, tab.data());
    for (uint32_t seed : SEEDS)
      for (uint64_t start : STARTS) {
        uint32_t base[POW_RAND_WORDS];
        state_at(seed, start, base);
        for (int k = 0; k < 25; ++k) {
          static const uint32_t corners[5][2] = {{0, 0}, {0, 255}, {1, 0}, {255, 0}, {255, 255}};
          const uint32_t w = k < 5 ? corners[k][0] : lcg() % POW_RAND_MAX_WG;
          const uint32_t l = k < 5 ? corners[k][1] : lcg() % 256u;
          uint32_t x[POW_RAND_WORDS], col[POW_RAND_WORDS];
          pow_rand_apply(B + w * POW_RAND_WORDS, base, x);
          for (uint32_t i = 0; i < POW_RAND_WORDS; ++i) col[i] = A[i * 256u + l];  // word-major
          pow_rand_apply(col, x, x);
          char got[POW_NONCE_SIZE], want[POW_NONCE_SIZE];
          pow_rand_nonce(x, got);
          const int rc = pow_rand_nonces(seed, start + (uint64_t)T * (256u * w + l), 1, want);
          CHECK(rc == POW_OK && memcmp(got, want, POW_NONCE_SIZE) == 0,
                "tables T=%u seed=%u start=%llu w=%u l=%u: \"%.9s\", pow_rand_nonces gives \"%.9s\"", T, seed,
                (unsigned long long)start, w, l, got, want);
        }
      }
  }
}

// ---- c ----
void lane_walk() {
  const uint32_t seed = 1700000003u;
  const uint64_t start = 1234577;
  std::vector<uint32_t> tab(POW_RAND_TAB_WORDS);
  const uint32_t* const A = tab.data();
  const uint32_t* const B = tab.data() + POW_RAND_WORDS * 256u;
  uint32_t launch_state[POW_RAND_WORDS];
  state_at(seed, start, launch_state);
  const uint32_t most = 3u * 3u * 256u * 64u + 5u;
  std::vector<char> want((size_t)most * POW_NONCE_SIZE);
  if (pow_rand_nonces(seed, start, most, want.data()) != POW_OK) {
    CHECK(false, "pow_rand_nonces: %s", pow_last_error());
    return;
  }
  const uint32_t Ts[] = {1, 4, 64};
  for (uint32_t nwg = 1; nwg <= 3; ++nwg)
    for (uint32_t T : Ts) {
      const uint32_t G = nwg * 256u;
      pow_rand_tables(T, tab.data());
      uint32_t step[POW_RAND_WORDS];
      pow_rand_power(9ull * T * ((uint64_t)G - 1u), step);  // restated, as the walk below: not pow_mine_rand's
      const uint32_t counts[] = {1, T - 1, T, T + 1, G * T - 1, G * T, G * T + 1, 3 * G * T + 5};
      for (uint32_t count : counts) {
        if (count == 0) continue;  // T - 1 of T = 1
        std::vector<uint8_t> seen(count, 0);
        long wrong_nonce = 0, outside = 0;
        for (uint32_t part = 0; part < nwg; ++part)
          for (uint32_t tid = 0; tid < 256u; ++tid) {
            uint32_t x[POW_RAND_WORDS], col[POW_RAND_WORDS];
            pow_rand_apply(B + part * POW_RAND_WORDS, launch_state, x);
            for (uint32_t i = 0; i < POW_RAND_WORDS; ++i) col[i] = A[i * 256u + tid];
            pow_rand_apply(col, x, x);
            // pow_rand.hip's walk, without the early stop
            const uint32_t hop_by = nwg * 256u * T - T;
            uint32_t rel = (part * 256u + tid) * T;
            uint32_t in_run = 0;
            bool go = rel < count;
            while (go) {
              char nonce[POW_NONCE_SIZE];
              pow_rand_nonce(x, nonce);
              if (rel >= count)
                ++outside;
              else {
                if (seen[rel] < 255) ++seen[rel];
                if (memcmp(nonce, want.data() + (size_t)rel * POW_NONCE_SIZE, POW_NONCE_SIZE) != 0) ++wrong_nonce;
              }
              ++rel;
              const bool hop = ++in_run == T;
              if (hop) {
                in_run = 0;
                rel += hop_by;
              }
              go = rel < count;
              if (go && hop) pow_rand_apply(step, x, x);
            }
          }
        const long once = std::count(seen.begin(), seen.end(), 1);
        CHECK(once == (long)count && outside == 0, "walk nwg=%u T=%u count=%u: %ld trials visited exactly once, %ld outside",
              nwg, T, count, once, outside);
        CHECK(wrong_nonce == 0, "walk nwg=%u T=%u count=%u: %ld visits drew another nonce than pow_rand_nonces", nwg, T,
              count, wrong_nonce);
      }
    }
}

// ---- d ----
void jumps_and_digits() {
  const uint32_t runs[] = {1, 31, 1024}, nwgs[] = {1, 256};
  const uint64_t starts[] = {0, 1, (1ull << 56) - 1}, per_launch[] = {1, 31ull * 256, 1ull << 26};
  for (uint32_t run : runs)
    for (uint32_t nwg : nwgs)
      for (uint64_t start : starts)
        for (uint64_t per : per_launch) {
          uint32_t got[3][POW_RAND_WORDS], want[3][POW_RAND_WORDS];
          memset(got, 0xA5, sizeof got);
          pow_rand_jumps(run, nwg, start, per, got[0], got[1], got[2]);
          pow_rand_power(9ull * run * ((uint64_t)nwg * 256u - 1u), want[0]);
          pow_rand_power(9ull * start, want[1]);
          pow_rand_power(9ull * per, want[2]);
          CHECK(memcmp(got, want, sizeof got) == 0, "jumps run=%u nwg=%u start=%llu per_launch=%llu", run, nwg,
                (unsigned long long)start, (unsigned long long)per);
        }
  // digit_of against digit_char, which pow_nonce_from_counter writes: its last character is digit ctr % 62
  bool in_alphabet[256] = {false};
  for (int k = 0; k < 62; ++k) {
    char nonce[POW_NONCE_SIZE];
    const bool ok = pow_nonce_from_counter((uint64_t)k, nonce) == POW_OK;
    CHECK(ok && digit_of(nonce[POW_NONCE_SIZE - 2]) == k, "digit_of('%c') = %d, digit %d", nonce[POW_NONCE_SIZE - 2],
          digit_of(nonce[POW_NONCE_SIZE - 2]), k);
    if (ok) in_alphabet[(uint8_t)nonce[POW_NONCE_SIZE - 2]] = true;
  }
  CHECK(std::count(in_alphabet, in_alphabet + 256, true) == 62, "62 distinct characters");
  for (int b = 0; b < 256; ++b)
    if (!in_alphabet[b]) CHECK(digit_of((char)b) == -1, "digit_of(byte %d) = %d", b, digit_of((char)b));
}

}  // namespace

int main() {
  plan_sweep();
  tables();
  lane_walk();
  jumps_and_digits();
  printf("%ld checks, %ld failed\n", checks, failed);
  return failed ? 1 : 0;
}
