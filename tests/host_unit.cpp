// CPU unit program of the HIP-free host code (csrc/pow_host.cpp): links that
// file alone, no GPU, no HIP.  tests/test_host_unit.py builds it under
// ASan/UBSan, feeds it tests/golden/golden.json as text lines on stdin and
// requires exit status 0:
//   T <name> <index> <owner> <difficulty> <created_at> <prev hex, 512>
//   D <template> <counter> <digest hex> <solves_d9: 0|1>
//   R <index> <owner> <difficulty> <created_at> <nonce hex, 20> <prev hex, 512> <digest hex>
// The SHA-256 here (round, schedule) is the test's own plain restatement of
// FIPS 180-4; K comes from PowConsts::k, which the digest checks pin.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "pow_host.h"

namespace {

int g_failed = 0, g_checks = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    ++g_checks;                                            \
    if (!(cond)) {                                         \
      ++g_failed;                                          \
      fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); \
      fprintf(stderr, __VA_ARGS__);                        \
      fputc('\n', stderr);                                 \
    }                                                      \
  } while (0)

const uint32_t IV[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
const uint64_t P62_8 = 218340105584896ull;  // 62^8

uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
uint32_t s0(uint32_t x) { return rotr(x, 7) ^ rotr(x, 18) ^ (x >> 3); }
uint32_t s1(uint32_t x) { return rotr(x, 17) ^ rotr(x, 19) ^ (x >> 10); }

// One round on the working variables s[0..7] = a..h, kw = K[i] + W[i].
void sha_round(uint32_t s[8], uint32_t kw) {
  const uint32_t a = s[0], b = s[1], c = s[2], e = s[4], f = s[5], g = s[6];
  const uint32_t t1 = s[7] + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + kw;
  const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
  for (int i = 7; i > 0; --i) s[i] = s[i - 1];
  s[4] += t1;
  s[0] = t1 + t2;
}

// One chunk: 64 rounds over its K+W words, then the feed-forward.
void compress(uint32_t h[8], const uint32_t kw[64]) {
  uint32_t s[8];
  memcpy(s, h, sizeof s);
  for (int i = 0; i < 64; ++i) sha_round(s, kw[i]);
  for (int i = 0; i < 8; ++i) h[i] += s[i];
}

std::string hex_of(const uint32_t h[8]) {
  char hex[65];
  digest_out(h, nullptr, hex);
  return hex;
}

void unhex(const char* hex, char* out, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    unsigned v = 0;
    if (sscanf(hex + 2 * i, "%2x", &v) != 1) {
      fprintf(stderr, "bad hex input\n");
      exit(2);
    }
    out[i] = (char)v;
  }
}

pow_block make_block(const char* index, const char* owner, const char* diff, const char* created, const char* prev_hex) {
  pow_block b;
  memset(&b, 0, sizeof b);
  b.index = (uint32_t)strtoull(index, nullptr, 10);
  b.node_owner_number = (uint32_t)strtoull(owner, nullptr, 10);
  b.difficulty = (uint32_t)strtoull(diff, nullptr, 10);
  b.created_at = strtoull(created, nullptr, 10);
  if (strlen(prev_hex) != 2 * POW_HASH_SIZE) {
    fprintf(stderr, "previous_block_hash: %zu hex chars\n", strlen(prev_hex));
    exit(2);
  }
  unhex(prev_hex, b.previous_block_hash, POW_HASH_SIZE);
  return b;
}

// pow_build_msg -> the five chunks' rounds -> hex.
std::string digest_via_msg(const pow_block& b) {
  PowMsg M;
  pow_build_msg(&b, &M);
  uint32_t h[8];
  memcpy(h, IV, sizeof h);
  for (int c = 0; c < 5; ++c) compress(h, M.kw[c]);
  return hex_of(h);
}

// pow_build_consts of the entry's template against the plain schedule of the
// block `b` = template + the nonce of `counter`.
void check_consts(const pow_block& tmpl, const pow_block& b, uint64_t counter, const char* want_hex) {
  PowConsts C;
  pow_build_consts(&tmpl, &C);
  PowMsg M;
  pow_build_msg(&b, &M);
  CHECK(memcmp(C.kw, M.kw[1], sizeof C.kw) == 0, "kw[0..3] != chunks 1-4 of the schedule (counter %" PRIu64 ")", counter);
  // chunk 0 as hashed: w0raw with the nonce words put in, expanded here
  const unsigned j = (unsigned)(counter % 62);
  uint32_t W[64];
  memcpy(W, C.w0raw, sizeof C.w0raw);
  CHECK(W[1] == 0 && W[2] == 0 && W[3] == C.w3lo && W[0] == C.w0, "w0raw placeholders");
  const uint8_t* n = (const uint8_t*)b.nonce;
  W[1] = (uint32_t)n[0] << 24 | (uint32_t)n[1] << 16 | (uint32_t)n[2] << 8 | n[3];
  W[2] = (uint32_t)n[4] << 24 | (uint32_t)n[5] << 16 | (uint32_t)n[6] << 8 | n[7];
  W[3] = (uint32_t)n[8] << 24 | C.w3lo;
  for (int i = 16; i < 64; ++i) W[i] = s1(W[i - 2]) + W[i - 7] + s0(W[i - 15]) + W[i - 16];
  uint32_t kw0[64];
  for (int i = 0; i < 64; ++i) kw0[i] = C.k[i] + W[i];
  CHECK(memcmp(kw0, M.kw[0], sizeof kw0) == 0, "chunk 0 from w0raw + k != pow_build_msg (counter %" PRIu64 ")", counter);
  uint32_t h[8];
  memcpy(h, IV, sizeof h);
  compress(h, kw0);
  for (int c = 0; c < 4; ++c) compress(h, C.kw[c]);
  CHECK(hex_of(h) == want_hex, "w0raw + k + kw digest %s != %s", hex_of(h).c_str(), want_hex);
  // st0: the working variables after round 0 (uniform: W0 only)
  uint32_t s[8];
  memcpy(s, IV, sizeof s);
  sha_round(s, C.k[0] + W[0]);
  CHECK(memcmp(s, C.st0, sizeof s) == 0, "st0");
  for (int i = 4; i < 16; ++i) CHECK(C.kw0[i] == C.k[i] + W[i], "kw0[%d]", i);
  // W16..W31 from the folded terms (pow_template.h)
  CHECK(C.w3[j] == W[3] && C.kw3[j] == C.k[3] + W[3], "w3/kw3[%u]", j);
  uint32_t R[32];
  memcpy(R, W, 16 * sizeof(uint32_t));
  R[16] = C.u16 + s0(W[1]);
  R[17] = C.u17 + s0(W[2]) + W[1];
  R[18] = s1(R[16]) + W[2] + C.u18[j];
  R[19] = s1(R[17]) + C.u19 + C.w3[j];
  R[20] = s1(R[18]) + C.u20;
  R[21] = s1(R[19]) + C.u21;
  R[22] = s1(R[20]) + C.u22;
  R[23] = s1(R[21]) + R[16] + C.u23;
  R[24] = s1(R[22]) + R[17] + C.u24;
  for (int k = 0; k < 6; ++k) R[25 + k] = s1(R[23 + k]) + R[18 + k] + C.u25[k];
  R[31] = s1(R[29]) + R[24] + s0(R[16]) + C.w15;
  for (int i = 16; i < 32; ++i) CHECK(R[i] == W[i], "W%d from the folded terms (counter %" PRIu64 ")", i, counter);
}

uint32_t want_thr(unsigned d) { return d < 32 ? (uint32_t)((1ull << (32 - d)) - 1) : 0u; }

void check_launch(uint64_t start, uint64_t count, unsigned diff) {
  PowLaunch L;
  CHECK(make_launch(start, count, diff, 7, 2, &L) == POW_OK, "make_launch(%" PRIu64 ", %" PRIu64 ")", start, count);
  uint64_t p = 0;
  for (int i = 0; i < 8; ++i) {
    CHECK(L.base_digit[i] < 62, "digit");
    p = p * 62 + L.base_digit[i];
  }
  CHECK(L.off0 < 62 && p == start / 62 && p * 62 + L.off0 == start, "prefix digits of %" PRIu64, start);
  CHECK(L.n_prefix == (L.off0 + count + 61) / 62, "n_prefix of (%" PRIu64 ", %" PRIu64 ")", start, count);
  CHECK(L.count == count && L.diff == diff && L.thr == want_thr(diff) && L.cap == 7 && L.mode == 2, "PowLaunch fields");
  PowLaunchLat Q;
  memset(&Q, 0xA5, sizeof Q);
  make_launch_lat(start, count, diff, &Q);
  p = 0;
  for (int i = 0; i < 9; ++i) {
    CHECK(Q.base_digit[i] < 62, "digit");
    p = p * 62 + Q.base_digit[i];
  }
  CHECK(p == start, "digits of %" PRIu64, start);
  CHECK(Q.count == count && Q.diff == diff && Q.thr == want_thr(diff), "PowLaunchLat fields");
  CHECK(Q.seq == 0 && Q.nwg == 0 && Q.watch.board == nullptr && Q.watch.watch_epoch == 0, "PowLaunchLat rest zeroed");
}

void check_launches() {
  const uint64_t counts[] = {1, 62, 1ull << 32};
  uint64_t starts[5 + 1000] = {0, 61, 62, P62_8 - 1, POW_COUNTER_LIMIT - (1ull << 32)};
  uint64_t x = 0x9E3779B97F4A7C15ull;  // xorshift64, fixed seed
  for (int i = 5; i < 5 + 1000; ++i) {
    x ^= x << 13, x ^= x >> 7, x ^= x << 17;
    starts[i] = x % POW_COUNTER_LIMIT;
  }
  for (uint64_t s : starts)
    for (uint64_t c : counts) check_launch(s, c, 9);
  for (unsigned d : {0u, 1u, 9u, 31u, 32u, 33u, 256u}) check_launch(12345, 62, d);
  PowLaunch L;
  const uint64_t np_max = 0xFFFFFFFFull - (1u << 26);
  CHECK(make_launch(0, np_max * 62, 9, 0, 0, &L) == POW_OK && L.n_prefix == np_max, "largest launch");
  CHECK(make_launch(0, np_max * 62 + 1, 9, 0, 0, &L) == POW_EINVAL && !strcmp(pow_last_error(), "launch too large"),
        "launch too large: %s", pow_last_error());
  CHECK(make_launch(61, np_max * 62 - 60, 9, 0, 0, &L) == POW_EINVAL, "launch too large by off0");
}

void check_edges() {
  char n[POW_NONCE_SIZE];
  const struct { uint64_t c; const char* s; } nonces[] = {
      {0, "aaaaaaaaa"}, {61, "aaaaaaaa9"}, {62, "aaaaaaaba"}, {POW_COUNTER_LIMIT - 1, "999999999"}};
  for (const auto& e : nonces) {
    memset(n, 0x7F, sizeof n);
    CHECK(pow_nonce_from_counter(e.c, n) == POW_OK && n[9] == 0 && !strcmp(n, e.s), "nonce of %" PRIu64, e.c);
  }
  CHECK(pow_nonce_from_counter(POW_COUNTER_LIMIT, n) == POW_EINVAL && !strcmp(pow_last_error(), "counter >= 62^9"),
        "nonce refusal at 62^9");
  CHECK(pow_nonce_from_counter(0, nullptr) == POW_EINVAL, "null nonce");
  pow_block b;
  memset(&b, 0, sizeof b);
  b.index = 300;
  b.node_owner_number = 0x1FF;
  b.created_at = 0x1000000FEull;
  uint8_t m[POW_MSG_BYTES];
  CHECK(pow_block_to_bytes(&b, m) == POW_OK && m[0] == 0x2C && m[1] == 0xFF && m[3] == 0xFE, "low bytes of the header");
  CHECK(check_range(&b, POW_COUNTER_LIMIT - 1, 1, 9) == POW_OK, "last counter");
  CHECK(check_range(&b, 0, POW_COUNTER_LIMIT, 256) == POW_OK, "whole space");
  CHECK(check_range(&b, POW_COUNTER_LIMIT - 1, 2, 9) == POW_EINVAL, "one past 62^9");
  CHECK(check_range(&b, 0, POW_COUNTER_LIMIT + 1, 9) == POW_EINVAL, "count past 62^9");
  CHECK(check_range(&b, POW_COUNTER_LIMIT, 0, 9) == POW_EINVAL && !strcmp(pow_last_error(), "counter range past 62^9"),
        "start at 62^9");
  CHECK(check_range(&b, 1, ~0ull, 9) == POW_EINVAL, "start + count wraps");
  CHECK(check_range(&b, 0, 1, 257) == POW_EINVAL, "d > 256");
  CHECK(check_range(nullptr, 0, 1, 9) == POW_EINVAL, "null template");
  CHECK(pow_set_error(POW_ECOMM, "x") == POW_ECOMM && !strcmp(pow_last_error(), "x"), "pow_set_error");
  const uint64_t t = mono_ns();
  CHECK(mono_ns() >= t, "mono_ns");
}

}  // namespace

int main() {
  std::map<std::string, pow_block> templates;
  static char line[4096];
  int n_digests = 0, n_random = 0;
  while (fgets(line, sizeof line, stdin)) {
    char* f[8] = {nullptr};
    int nf = 0;
    for (char* tok = strtok(line, " \n"); tok && nf < 8; tok = strtok(nullptr, " \n")) f[nf++] = tok;
    if (nf == 0) continue;
    if (!strcmp(f[0], "T") && nf == 7) {
      templates[f[1]] = make_block(f[2], f[3], f[4], f[5], f[6]);
    } else if (!strcmp(f[0], "D") && nf == 5 && templates.count(f[1])) {
      const pow_block& tmpl = templates[f[1]];
      const uint64_t counter = strtoull(f[2], nullptr, 10);
      pow_block b = tmpl;
      CHECK(pow_nonce_from_counter(counter, b.nonce) == POW_OK, "counter %" PRIu64, counter);
      const std::string got = digest_via_msg(b);
      CHECK(got == f[3], "%s counter %" PRIu64 ": %s != %s", f[1], counter, got.c_str(), f[3]);
      CHECK(pow_solves_problem(got.c_str(), 9) == atoi(f[4]), "solves_d9 of %s", got.c_str());
      check_consts(tmpl, b, counter, f[3]);
      ++n_digests;
    } else if (!strcmp(f[0], "R") && nf == 8 && strlen(f[5]) == 2 * POW_NONCE_SIZE) {
      pow_block b = make_block(f[1], f[2], f[3], f[4], f[6]);
      unhex(f[5], b.nonce, POW_NONCE_SIZE);
      const std::string got = digest_via_msg(b);
      CHECK(got == f[7], "random block %d: %s != %s", n_random, got.c_str(), f[7]);
      ++n_random;
    } else {
      fprintf(stderr, "bad input line: %s ...\n", f[0]);
      return 2;
    }
  }
  check_launches();
  check_edges();
  printf("host_unit: %zu templates, %d digests, %d random blocks, %d checks, %d failed\n", templates.size(), n_digests,
         n_random, g_checks, g_failed);
  return g_failed ? 1 : 0;
}
