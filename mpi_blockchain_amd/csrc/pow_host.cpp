// Host code of the C ABI that needs no GPU (pow_host.h): the error string, the
// clock, the per-template precompute, the launch splitting, the plans of the
// fused mining calls and the host-side helpers of include/pow_gpu.h.  No HIP
// header: tests/host_unit.cpp links this file alone and runs it on the CPU.
#include "pow_host.h"

#include <time.h>

#include <algorithm>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>

static_assert(sizeof(pow_block) == 552, "pow_block must match block.h:17-25 (LP64)");
static_assert(offsetof(pow_block, created_at) == 16, "layout");
static_assert(offsetof(pow_block, nonce) == 24, "layout");
static_assert(offsetof(pow_block, previous_block_hash) == 34, "layout");
static_assert(offsetof(pow_block, block_hash) == 290, "layout");
static_assert(sizeof(PowConsts) % 4 == 0 && sizeof(PowConsts) < 4096, "consts");
static_assert(offsetof(PowConsts, kw0) == 4 * PC_KW0, "PC_KW0");
static_assert(offsetof(PowConsts, u20) == 4 * PC_U20, "PC_U20");
static_assert(offsetof(PowConsts, u21) == 4 * (PC_U20 + 1), "PC_U21");
static_assert(offsetof(PowConsts, u22) == 4 * (PC_U20 + 2), "PC_U22");
static_assert(offsetof(PowConsts, u25) == 4 * PC_U25, "PC_U25");
static_assert(offsetof(PowConsts, kw3) == 4 * PC_KW3, "PC_KW3");
static_assert(offsetof(PowConsts, u18) == 4 * PC_U18, "PC_U18");
static_assert(offsetof(PowConsts, w3) == 4 * PC_W3, "PC_W3");
static_assert(offsetof(PowConsts, k) == 4 * PC_K, "PC_K");
static_assert(offsetof(PowConsts, st0) == 4 * PC_ST0, "PC_ST0");
static_assert(offsetof(PowConsts, w0raw) == 4 * PC_WRAW, "PC_WRAW");
static_assert(offsetof(PowConstsLat, st0) == 4 * LC_ST0 && offsetof(PowConstsLat, kw0) == 4 * LC_KW0 &&
                  offsetof(PowConstsLat, k) == 4 * LC_K && offsetof(PowConstsLat, w0raw) == 4 * LC_WRAW,
              "LC_*");

namespace {

thread_local std::string g_err;

// ---------------- host SHA-256 pieces for the template precompute ----------------
// (FIPS 180-4 / picosha2.h:46-136; only the parts needed to fold constants)
const uint32_t kK[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
    0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
    0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
    0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
    0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
    0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
    0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
    0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
const uint32_t kIV[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a,
                         0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};

inline uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
inline uint32_t ssig0(uint32_t x) { return rotr(x, 7) ^ rotr(x, 18) ^ (x >> 3); }
inline uint32_t ssig1(uint32_t x) { return rotr(x, 17) ^ rotr(x, 19) ^ (x >> 10); }

// block.cpp:61-72 alphabet.
inline char digit_char(unsigned d) {
  return d < 26 ? (char)('a' + d) : d < 52 ? (char)('A' + d - 26) : (char)('0' + d - 52);
}

// One 64-byte chunk's message schedule with K folded in: kw[i] = K[i] + W[i]
// (the rounds that consume it run on the GPU).
void chunk_kw(uint32_t kw[64], const uint8_t* chunk) {
  uint32_t w[64];
  for (int i = 0; i < 16; ++i) w[i] = be32(chunk + 4 * i);
  for (int i = 16; i < 64; ++i) w[i] = ssig1(w[i - 2]) + w[i - 7] + ssig0(w[i - 15]) + w[i - 16];
  for (int i = 0; i < 64; ++i) kw[i] = kK[i] + w[i];
}

// The n base-62 digits of v, most significant first.
void split62(uint64_t v, uint32_t* digit, int n) {
  for (int i = n - 1; i >= 0; --i) {
    digit[i] = (uint32_t)(v % 62);
    v /= 62;
  }
}

// d <= 32: a digest solves iff H0 <= thr; d > 32: thr = 0 (the full test).
uint32_t diff_thr(unsigned diff) { return diff >= 32 ? 0u : (0xFFFFFFFFu >> diff); }

}  // namespace

// digit_char's inverse.
int digit_of(char c) {
  return c >= 'a' && c <= 'z' ? c - 'a' : c >= 'A' && c <= 'Z' ? c - 'A' + 26 : c >= '0' && c <= '9' ? c - '0' + 52 : -1;
}

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

int pow_set_error(int code, const char* msg) { return fail(code, "%s", msg); }

uint64_t mono_ns() {
  timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return (uint64_t)t.tv_sec * 1000000000ull + (uint64_t)t.tv_nsec;
}

uint32_t be32(const uint8_t* p) {
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}

void padded_message(const pow_block* b, uint8_t m[320]) {
  memset(m, 0, 320);
  pow_block_to_bytes(b, m);
  m[POW_MSG_BYTES] = 0x80;
  const uint64_t bits = (uint64_t)POW_MSG_BYTES * 8;  // 2160
  for (int i = 0; i < 8; ++i) m[319 - i] = (uint8_t)(bits >> (8 * i));
}

void pow_build_consts(const pow_block* tmpl, PowConsts* C) {
  memset(C, 0, sizeof *C);
  pow_block b = *tmpl;
  memset(b.nonce, 0, sizeof b.nonce);  // nonce bytes are per trial; nonce[9] stays NUL
  uint8_t m[320];
  padded_message(&b, m);
  for (int c = 1; c < 5; ++c) chunk_kw(C->kw[c - 1], m + 64 * c);
  uint32_t W[16];
  for (int i = 0; i < 16; ++i) W[i] = be32(m + 4 * i);
  C->w0 = W[0];
  C->w3lo = W[3] & 0x00FFFFFFu;  // [nonce[9]=0, prev[0], prev[1]]
  for (int i = 4; i < 16; ++i) C->kw0[i] = kK[i] + W[i];
  // round 0 of chunk 0 (uniform)
  uint32_t a = kIV[0], bb = kIV[1], c = kIV[2], d = kIV[3], e = kIV[4], f = kIV[5], g = kIV[6], h = kIV[7];
  {
    uint32_t S1 = rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25);
    uint32_t chv = (e & f) ^ (~e & g);
    uint32_t t1 = h + S1 + chv + kK[0] + W[0];
    uint32_t S0 = rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22);
    uint32_t mj = (a & bb) ^ (a & c) ^ (bb & c);
    h = g; g = f; f = e; e = d + t1; d = c; c = bb; bb = a; a = t1 + S0 + mj;
  }
  const uint32_t st[8] = {a, bb, c, d, e, f, g, h};
  memcpy(C->st0, st, sizeof st);
  C->u16 = ssig1(W[14]) + W[9] + W[0];
  C->u17 = ssig1(W[15]) + W[10];
  C->u19 = W[12] + ssig0(W[4]);
  C->u20 = W[13] + ssig0(W[5]) + W[4];
  C->u21 = W[14] + ssig0(W[6]) + W[5];
  C->u22 = W[15] + ssig0(W[7]) + W[6];
  C->u23 = ssig0(W[8]) + W[7];
  C->u24 = ssig0(W[9]) + W[8];
  for (int k = 0; k < 6; ++k) C->u25[k] = ssig0(W[10 + k]) + W[9 + k];
  C->w15 = W[15];
  memcpy(C->k, kK, sizeof kK);
  memcpy(C->w0raw, W, sizeof W);  // nonce words zero: W1 = W2 = 0, W3 = w3lo
  for (unsigned j = 0; j < POW_J; ++j) {
    const uint32_t w3 = ((uint32_t)(uint8_t)digit_char(j) << 24) | C->w3lo;
    C->w3[j] = w3;
    C->kw3[j] = kK[3] + w3;
    C->u18[j] = ssig0(w3) + W[11];
  }
}

void pow_build_msg(const pow_block* b, PowMsg* M) {
  uint8_t m[320];
  padded_message(b, m);
  for (int c = 0; c < 5; ++c) chunk_kw(M->kw[c], m + 64 * c);
}

void digest_out(const uint32_t* h, uint8_t* digest, char* hex) {
  static const char hexd[] = "0123456789abcdef";
  uint8_t d[32];
  for (int k = 0; k < 8; ++k) {
    d[4 * k] = (uint8_t)(h[k] >> 24);
    d[4 * k + 1] = (uint8_t)(h[k] >> 16);
    d[4 * k + 2] = (uint8_t)(h[k] >> 8);
    d[4 * k + 3] = (uint8_t)h[k];
  }
  if (digest) memcpy(digest, d, 32);
  if (hex) {
    for (int k = 0; k < 32; ++k) {
      hex[2 * k] = hexd[d[k] >> 4];
      hex[2 * k + 1] = hexd[d[k] & 15];
    }
    hex[64] = 0;
  }
}

int check_range(const pow_block* tmpl, uint64_t start, uint64_t count, unsigned diff) {
  if (!tmpl) return fail(POW_EINVAL, "null template");
  if (diff > 256) return fail(POW_EINVAL, "difficulty %u > 256 bits", diff);
  if (start >= POW_COUNTER_LIMIT || count > POW_COUNTER_LIMIT - start)
    return fail(POW_EINVAL, "counter range past 62^9");
  return POW_OK;
}

int make_launch(uint64_t start, uint64_t count, unsigned diff, uint32_t cap, uint32_t mode,
                PowLaunch* L) {
  memset(L, 0, sizeof *L);
  const uint64_t P0 = start / POW_J;
  L->off0 = (uint32_t)(start - P0 * POW_J);
  const uint64_t np = (L->off0 + count + POW_J - 1) / POW_J;
  if (np > 0xFFFFFFFFull - (1u << 26)) return fail(POW_EINVAL, "launch too large");
  L->n_prefix = (uint32_t)np;
  split62(P0, L->base_digit, 8);
  L->count = count;
  L->diff = diff;
  L->thr = diff_thr(diff);
  L->cap = cap;
  L->mode = mode;
  return POW_OK;
}

void make_launch_lat(uint64_t start, uint64_t count, unsigned diff, PowLaunchLat* L) {
  memset(L, 0, sizeof *L);
  split62(start, L->base_digit, 9);
  L->count = count;
  L->diff = diff;
  L->thr = diff_thr(diff);
}

void pow_race_plan(unsigned diff, uint32_t n_rivals, uint64_t ctr_count, uint32_t cu_count, unsigned lanes_log2,
                   unsigned batch_override, PowRacePlan* p) {
  const uint64_t R = n_rivals < 1 ? 1 : n_rivals;
  const uint64_t cus = cu_count < 1 ? 1 : cu_count;
  const unsigned d = diff > 32 ? 32 : diff;
  // Lanes over all rivals for 2^lanes_log2 times the 2^d trials a height is
  // expected to cost, split evenly: a rival gets no more lanes than its window
  // has counters, at least one workgroup, and no more workgroups than its share
  // of one per CU.
  const uint64_t total = 1ull << (d + (lanes_log2 > 8 ? 8 : lanes_log2));
  uint64_t lanes = (total + R - 1) / R;
  if (lanes > ctr_count) lanes = ctr_count;
  uint64_t nwg = (lanes + 255) / 256;
  const uint64_t share = cus / R < 1 ? 1 : cus / R;
  if (nwg > share) nwg = share;
  if (nwg < 1) nwg = 1;
  p->nwg_r = (uint32_t)nwg;
  // A batch is about 2^26 expected trials (a handful of ms: the cancel
  // latency), at most 64 heights, and the largest for which the windows of all
  // rivals of all its heights hold 2^38 counters at most; never below one.
  uint64_t batch = batch_override ? batch_override : 1ull << (26 - (d > 26 ? 26 : d));
  if (batch > 64) batch = 64;
  const uint64_t per_height = R * (ctr_count < 1 ? 1 : ctr_count);  // <= 2^40
  const uint64_t cap = (1ull << 38) / per_height;
  if (batch > cap) batch = cap;
  if (batch < 1) batch = 1;
  p->batch = (uint32_t)batch;
}

namespace {
// Workgroups for 2^lanes_log2 times the expected 2^d trials: no more lanes than
// the window has counters, no more workgroups than `most`, never below one.
uint64_t nwg_for(unsigned d, unsigned lanes_log2, uint64_t ctr_count, uint64_t most) {
  const uint64_t lanes = std::min<uint64_t>(1ull << (d + lanes_log2), ctr_count);
  return std::max<uint64_t>(1, std::min<uint64_t>((lanes + 255) / 256, most));
}
}  // namespace

PowChainPlan pow_chain_plan(unsigned diff, uint64_t ctr_count, uint32_t grid_max, unsigned lanes_log2,
                            unsigned batch_override) {
  const unsigned d = std::min(diff, 32u);
  // The grid follows the difficulty: lanes for four times the expected 2^d
  // trials (a block then costs one trial's latency but for 1 in e^4; at d = 9
  // and 13 two times measured 1.4 and 0.6 us per block slower, eight times 0.3
  // and 2.2 us: more workgroups to start and to count out), no more than the
  // window has counters or the chip takes at one wave per SIMD; the lanes of a
  // full grid walk on through the window.
  PowChainPlan p;
  p.nwg = (uint32_t)nwg_for(d, std::min(lanes_log2, 8u), ctr_count, grid_max);
  // A batch is about 2^26 expected trials (a handful of ms: the cancel latency).
  const uint64_t batch = batch_override ? batch_override : 1ull << (26 - std::min(d, 26u));
  p.batch = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(batch, POW_CHAIN_MAX_BATCH));
  return p;
}

PowBatchPlan pow_batch_plan(unsigned diff, uint64_t n, uint64_t ctr_count, uint32_t cu_count, int lanes_log2,
                            unsigned tile_override) {
  const unsigned d = std::min(diff, 32u);
  const uint64_t window = std::max<uint64_t>(1, ctr_count), cus = std::max(1u, cu_count);
  // Templates per launch: about 2^26 expected trials (a handful of ms: the
  // cancel latency), a grid of at most 2^16 workgroups, and windows of at most
  // 2^38 counters in all, which keeps the watchdog's 2 ns per counter a bound
  // worth having (550 s, K4's own worst case).
  uint64_t tile = tile_override ? tile_override : (1ull << 26) / std::min<uint64_t>(1ull << std::min(d, 26u), window);
  tile = std::min<uint64_t>(tile, (1ull << 38) / window);
  tile = std::max<uint64_t>(1, std::min<uint64_t>(tile, POW_BATCH_MAX_TILE));
  // Lanes for 2^lanes_log2 times the expected 2^d trials of a template: no
  // more than the window has counters or the chip takes at one wave per SIMD.
  // Four times, as K4, while the launch leaves CUs idle (a template then costs
  // one trial's latency but for 1 in e^4); every lane computes at least one
  // trial, so once the launch's workgroups exceed one per CU the surplus
  // lanes are only surplus work: twice, then once the expected trials
  // (d = 13, 64 templates: 8.8 us per template at four times, 4.1 at once).
  unsigned ll = lanes_log2 < 0 ? 2u : std::min((unsigned)lanes_log2, 8u);
  if (lanes_log2 < 0)
    while (ll > 0 && std::min(tile, n) * nwg_for(d, ll, window, cus) > cus) --ll;
  PowBatchPlan p;
  p.nwg_t = (uint32_t)nwg_for(d, ll, window, cus);
  p.tile = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(tile, POW_BATCH_MAX_WG / p.nwg_t));
  return p;
}

// ---------------- glibc's TYPE_3 rand(), restated (block.cpp:61-72's source of nonces) ----------------

void pow_rand_seed(uint32_t seed, uint32_t x[POW_RAND_WORDS]) {
  uint32_t r[344];
  r[0] = seed ? seed : 1u;
  for (int i = 1; i < 31; ++i) {
    const int32_t w = (int32_t)r[i - 1];
    const int32_t hi = w / 127773, lo = w - hi * 127773;  // C division: toward zero
    int64_t v = 16807ll * lo - 2836ll * hi;
    if (v < 0) v += 2147483647;
    r[i] = (uint32_t)v;
  }
  for (int i = 31; i < 34; ++i) r[i] = r[i - 31];
  for (int i = 34; i < 344; ++i) r[i] = r[i - 31] + r[i - 3];
  memcpy(x, r + 313, POW_RAND_WORDS * sizeof(uint32_t));
}

uint32_t pow_rand_draw(uint32_t x[POW_RAND_WORDS]) {
  const uint32_t v = x[0] + x[28];
  memmove(x, x + 1, (POW_RAND_WORDS - 1) * sizeof(uint32_t));
  x[POW_RAND_WORDS - 1] = v;
  return v >> 1;
}

void pow_rand_mul(const uint32_t a[POW_RAND_WORDS], const uint32_t b[POW_RAND_WORDS], uint32_t out[POW_RAND_WORDS]) {
  uint32_t t[2 * POW_RAND_WORDS - 1] = {0};
  for (int i = 0; i < POW_RAND_WORDS; ++i)
    for (int j = 0; j < POW_RAND_WORDS; ++j) t[i + j] += a[i] * b[j];
  for (int k = 2 * POW_RAND_WORDS - 2; k >= POW_RAND_WORDS; --k) {  // x^k = x^(k-3) + x^(k-31)
    t[k - 3] += t[k];
    t[k - 31] += t[k];
  }
  memcpy(out, t, POW_RAND_WORDS * sizeof(uint32_t));
}

void pow_rand_power(uint64_t n, uint32_t c[POW_RAND_WORDS]) {
  uint32_t sq[POW_RAND_WORDS] = {0, 1u};  // x
  memset(c, 0, POW_RAND_WORDS * sizeof(uint32_t));
  c[0] = 1u;
  for (; n; n >>= 1) {
    if (n & 1u) pow_rand_mul(c, sq, c);
    pow_rand_mul(sq, sq, sq);
  }
}

void pow_rand_apply(const uint32_t c[POW_RAND_WORDS], const uint32_t x[POW_RAND_WORDS], uint32_t y[POW_RAND_WORDS]) {
  uint32_t e[2 * POW_RAND_WORDS - 1], out[POW_RAND_WORDS];
  memcpy(e, x, POW_RAND_WORDS * sizeof(uint32_t));
  for (int k = POW_RAND_WORDS; k < 2 * POW_RAND_WORDS - 1; ++k) e[k] = e[k - 31] + e[k - 3];
  for (int j = 0; j < POW_RAND_WORDS; ++j) {
    uint32_t s = 0;
    for (int i = 0; i < POW_RAND_WORDS; ++i) s += c[i] * e[i + j];
    out[j] = s;
  }
  memcpy(y, out, sizeof out);
}

void pow_rand_nonce(uint32_t x[POW_RAND_WORDS], char nonce[POW_NONCE_SIZE]) {
  for (int i = 0; i < POW_NONCE_SIZE - 1; ++i) nonce[i] = digit_char(pow_rand_draw(x) % 62u);
  nonce[POW_NONCE_SIZE - 1] = 0;  // block.cpp:71
}

PowRandPlan pow_rand_plan(unsigned diff, uint64_t trial_count, uint32_t cu_count, int lanes_log2, unsigned run_override,
                          unsigned launch_log2) {
  const unsigned d = std::min(diff, 32u);
  PowRandPlan p;
  p.launch = 1ull << std::min(launch_log2, 26u);  // 2^26: the cancel latency, a handful of ms
  const uint64_t n = std::max<uint64_t>(1, std::min(trial_count, p.launch));
  const uint64_t most = std::min<uint64_t>(std::max(1u, cu_count), POW_RAND_MAX_WG);
  // The grid is K4's: lanes for four times the expected 2^d trials, at most one workgroup per CU.
  p.nwg = (uint32_t)(lanes_log2 < 0 ? nwg_for(d, 2, n, most)
                                    : nwg_for(0, (unsigned)std::min(lanes_log2, 16), n, most));
  // One trial per lane while that grid covers four times the expected trials
  // (or the launch): a block then costs one trial's latency, as K4's.  Above
  // that a lane walks T consecutive trials per pass, so that one pass covers them.
  const uint64_t want = std::min<uint64_t>(4ull << d, n);
  uint32_t run = 1;
  if (run_override)
    while (2 * run <= std::min(run_override, POW_RAND_MAX_RUN)) run *= 2;
  else
    while (run < POW_RAND_MAX_RUN && (uint64_t)p.nwg * 256u * run < want) run *= 2;
  p.run = run;
  return p;
}

void pow_rand_tables(uint32_t run, uint32_t* tab) {
  uint32_t step[POW_RAND_WORDS], cur[POW_RAND_WORDS];
  uint32_t* const A = tab;
  uint32_t* const B = tab + POW_RAND_WORDS * 256u;
  pow_rand_power(9ull * run, step);
  pow_rand_power(0, cur);
  for (uint32_t l = 0; l < 256u; ++l) {
    for (int i = 0; i < POW_RAND_WORDS; ++i) A[i * 256u + l] = cur[i];
    pow_rand_mul(cur, step, cur);
  }
  memcpy(step, cur, sizeof step);  // x^(9 T 256)
  pow_rand_power(0, cur);
  for (uint32_t w = 0; w < POW_RAND_MAX_WG; ++w) {
    memcpy(B + w * POW_RAND_WORDS, cur, sizeof cur);
    pow_rand_mul(cur, step, cur);
  }
}

void pow_rand_jumps(uint32_t run, uint32_t nwg, uint64_t trial_start, uint64_t per_launch, uint32_t step[POW_RAND_WORDS],
                    uint32_t first[POW_RAND_WORDS], uint32_t to_next[POW_RAND_WORDS]) {
  pow_rand_power(9ull * run * ((uint64_t)nwg * 256u - 1u), step);
  pow_rand_power(9ull * trial_start, first);
  pow_rand_power(9ull * per_launch, to_next);
}

// ---------------- pow_find_seed (K9) ----------------

bool pow_seed_pack(const char* nonce, uint32_t w[2]) {
  uint32_t d[POW_NONCE_SIZE - 1];
  for (int i = 0; i < POW_NONCE_SIZE - 1; ++i) {
    const int digit = digit_of(nonce[i]);
    if (digit < 0) return false;
    d[i] = (uint32_t)digit;
  }
  w[0] = (d[0] << 24) | (d[1] << 18) | (d[2] << 12) | (d[3] << 6) | d[4];
  w[1] = (d[5] << 18) | (d[6] << 12) | (d[7] << 6) | d[8];
  return true;
}

PowSeedPlan pow_seed_plan(uint32_t n_seeds, uint64_t trial_count, uint32_t cu_count, unsigned run_override,
                          unsigned wg_override, unsigned launch_log2) {
  PowSeedPlan p;
  const uint64_t cap = 1ull << std::min(launch_log2, POW_SEED_LAUNCH_LOG2);  // pairs per launch: the cancel latency
  // A slice is at most 2^26 trials, K8's launch: with a pass of the grid below
  // 2^26 too, a lane's relative trial stays below 2^27.
  p.slice = std::max<uint64_t>(1, std::min<uint64_t>(trial_count, std::min<uint64_t>(1ull << 26, cap)));
  uint64_t tile = std::min<uint64_t>(std::max(1u, n_seeds), std::max<uint64_t>(1, cap / p.slice));
  // Workgroups per seed: eight per CU over the tile fill the chip, and none
  // whose first run (at the least T) would start past the slice.
  const uint64_t one = 256ull * POW_RAND_WORDS;
  uint64_t nwg = (8ull * std::max(1u, cu_count) + tile - 1) / tile;
  nwg = std::min(nwg, (p.slice + one - 1) / one);
  if (wg_override) nwg = wg_override;
  p.nwg = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(nwg, POW_RAND_MAX_WG));
  p.tile = (uint32_t)std::min<uint64_t>(tile, (1u << 16) / p.nwg);
  // T = 31 x 2^j: the largest at which one pass of the grid still lies inside
  // the slice, so that every lane has a run and hops as seldom as can be.
  uint32_t run = POW_RAND_WORDS;
  if (run_override)
    while (run < 32u * POW_RAND_WORDS && 2 * run <= run_override) run *= 2;
  else
    while (run < 32u * POW_RAND_WORDS && (uint64_t)p.nwg * 256u * (2 * run) <= p.slice) run *= 2;
  p.run = run;
  return p;
}

PowPoolPlan pow_pool_plan(uint32_t n, unsigned slots_log2) {
  PowPoolPlan p;
  // The lowest power of two that is at least 2 n; an override may go below it,
  // down to the lowest one that still leaves a slot empty.
  uint32_t least = 1;
  while (least < n + 1u) least *= 2;
  uint32_t slots = 2;
  while (slots < 2ull * n) slots *= 2;
  if (slots_log2) slots = std::max(least, 1u << std::min(slots_log2, 21u));
  p.slots = slots;
  p.rounds = pow_pool_rounds(n);
  const uint32_t bytes = (n + 3u) / 4u;  // n bytes in whole words
  uint32_t at = 0;
  auto take = [&](uint32_t words) {
    const uint32_t here = at;
    at += words;
    return here;
  };
  p.ctl = take(4);
  p.dig = take(8u * n);
  p.prev = take(8u * n);
  p.index = take(n);
  p.parent = take(n);
  for (int k = 0; k < 2; ++k) p.next[k] = take(n);
  for (int k = 0; k < 2; ++k) p.depth[k] = take(n);
  for (int k = 0; k < 2; ++k) p.bad[k] = take(n);
  p.status = take(bytes);
  p.kind = take(bytes);
  p.table = take(slots);
  p.words = at;
  return p;
}

PowPoolLivePlan pow_pool_live_plan(uint32_t cap) {
  PowPoolLivePlan p;
  p.cap = cap;
  const uint32_t bytes = (cap + 3u) / 4u;  // cap bytes in whole words
  uint32_t at = 0;
  auto take = [&](uint32_t words) {
    const uint32_t here = at;
    at += words;
    return here;
  };
  p.ctl = take(8);  // POW_POOL_LIVE_CTL_WORDS, and dig stays on 16 bytes
  p.dig = take(8u * cap);
  p.prev = take(8u * cap);
  p.index = take(cap);
  p.parent = take(cap);
  for (int k = 0; k < 2; ++k) p.next[k] = take(cap);
  for (int k = 0; k < 2; ++k) p.depth[k] = take(cap);
  for (int k = 0; k < 2; ++k) p.bad[k] = take(cap);
  p.status = take(bytes);
  p.kind = take(bytes);
  p.words = at;
  return p;
}

uint32_t pow_pool_live_first_cap(size_t reserve, unsigned first_cap) {
  const size_t want = reserve ? reserve : first_cap ? first_cap : POW_POOL_LIVE_FIRST_CAP;
  return (uint32_t)std::min<size_t>(want, POW_POOL_MAX_BLOCKS);
}

uint32_t pow_pool_live_grow(uint32_t cap, uint32_t need) {
  uint64_t c = std::max(1u, cap);
  while (c < need) c *= 2;
  return (uint32_t)std::min<uint64_t>(c, POW_POOL_MAX_BLOCKS);
}

uint32_t pow_pool_live_first_slots(uint32_t cap, unsigned slots_log2) {
  if (slots_log2) return 1u << std::min(slots_log2, 21u);
  return pow_pool_live_slots(2, cap);
}

uint32_t pow_pool_live_slots(uint32_t slots, uint32_t size) {
  if (size <= slots / 2u) return slots;
  uint32_t s = 2;
  while (s < 2ull * size) s *= 2;
  return s;
}

uint32_t pow_pool_rounds(uint32_t n) {
  uint32_t r = 0;
  while ((1ull << r) < n) ++r;
  return r;
}

uint32_t pow_pool_live_launches(uint32_t m, uint32_t size, bool rerank) {
  const uint32_t tiles = (m + (1u << 16) - 1u) >> 16;
  return tiles + 3u + pow_pool_rounds(m) + (rerank ? 3u + pow_pool_rounds(size) : 0u);
}

uint32_t pow_pool_prune_cap(uint32_t kept, uint32_t first_cap) {
  const uint32_t need = std::min(std::max(std::max(kept, first_cap), 1u), POW_POOL_MAX_BLOCKS);
  return 1u << pow_pool_rounds(need);
}

uint32_t pow_pool_prune_slots(uint32_t cap, uint32_t kept, unsigned slots_log2) {
  return pow_pool_live_slots(pow_pool_live_first_slots(cap, slots_log2), kept);
}

uint32_t pow_pool_prune_launches(uint32_t size, uint32_t kept, bool prune) {
  if (size == 0) return 0;
  return 3u + pow_pool_rounds(size) + (prune && kept != 0 && kept < size ? 3u : 0u);
}

uint32_t pow_pool_lift_rows(uint32_t n) {
  const uint32_t r = pow_pool_rounds(n);
  return r ? r - 1u : 0u;
}

uint64_t pow_pool_lift_bytes(uint32_t cap) { return 4ull * cap * pow_pool_lift_rows(cap); }

uint32_t pow_pool_lift_launches(uint32_t covered, uint32_t size, bool stale) {
  if (stale) return pow_pool_lift_rows(size);
  if (covered >= size) return 0;
  const uint32_t m = size - covered, have = pow_pool_lift_rows(covered);
  return (have ? (m <= POW_POOL_LIFT_SMALL ? 1u : have) : 0u) + (pow_pool_lift_rows(size) - have);
}

extern "C" {

const char* pow_last_error(void) { return g_err.c_str(); }

int pow_rand_nonces(uint32_t seed, uint64_t trial_start, size_t n, char* nonces) {
  if (trial_start > POW_RAND_TRIAL_LIMIT || n > POW_RAND_TRIAL_LIMIT - trial_start)
    return fail(POW_EINVAL, "trials past POW_RAND_TRIAL_LIMIT (2^56)");
  if (!nonces && n) return fail(POW_EINVAL, "null nonces");
  uint32_t x[POW_RAND_WORDS], jump[POW_RAND_WORDS];
  pow_rand_seed(seed, x);
  pow_rand_power(9ull * trial_start, jump);  // < 2^60
  pow_rand_apply(jump, x, x);
  for (size_t t = 0; t < n; ++t) pow_rand_nonce(x, nonces + t * POW_NONCE_SIZE);
  return POW_OK;
}

int pow_nonce_from_counter(uint64_t ctr, char nonce[POW_NONCE_SIZE]) {
  if (!nonce) return fail(POW_EINVAL, "null nonce");
  if (ctr >= POW_COUNTER_LIMIT) return fail(POW_EINVAL, "counter >= 62^9");
  for (int i = POW_NONCE_SIZE - 2; i >= 0; --i) {
    nonce[i] = digit_char((unsigned)(ctr % 62));
    ctr /= 62;
  }
  nonce[POW_NONCE_SIZE - 1] = 0;  // block.cpp:71
  return POW_OK;
}

int pow_block_to_bytes(const pow_block* b, uint8_t out[POW_MSG_BYTES]) {
  if (!b || !out) return fail(POW_EINVAL, "null");
  // block.cpp:81-84: std::string::operator+=(char) keeps the low byte (trap T1)
  out[0] = (uint8_t)b->index;
  out[1] = (uint8_t)b->node_owner_number;
  out[2] = (uint8_t)b->difficulty;
  out[3] = (uint8_t)b->created_at;
  memcpy(out + 4, b->nonce, POW_NONCE_SIZE);                        // block.cpp:85
  memcpy(out + 4 + POW_NONCE_SIZE, b->previous_block_hash, POW_HASH_SIZE);  // block.cpp:86
  return POW_OK;
}

int pow_solves_problem(const char* hex, unsigned diff_bits) {
  if (!hex) return 0;
  // block.cpp:28-58, 91-96: binary expansion of the hex string (toupper;
  // non-hex chars count as "1111"), first diff_bits chars must be '0'.
  const size_t len = strlen(hex);
  if ((size_t)diff_bits > 4 * len) return 0;
  for (unsigned i = 0; i < diff_bits; ++i) {
    char c = hex[i / 4];
    unsigned v;
    if (c >= '0' && c <= '9') v = (unsigned)(c - '0');
    else if ((c >= 'a' && c <= 'e') || (c >= 'A' && c <= 'E')) v = 10u + (unsigned)((c | 0x20) - 'a');
    else v = 15;
    if ((v >> (3 - i % 4)) & 1u) return 0;
  }
  return 1;
}

}  // extern "C"
