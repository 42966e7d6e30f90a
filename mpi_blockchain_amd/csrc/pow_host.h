// HIP-free host code of the miner (pow_host.cpp): the error string, the
// clock, the per-template precompute, the launch splitting and the plans of
// the fused mining calls (K4, K5, K6), and the reference's rand() stream with
// the plans of K8 and K9.  Pure integer code: it compiles with a
// plain C++ compiler and no ROCm include path, so tests/host_unit.cpp and
// tests/{race,fused}_plan_unit.cpp run it on the CPU under sanitizers.  Library-internal
// (pow_api.cpp, pow_group.cpp, pow_aql.cpp, pow_hooks.cpp); not part of the C
// ABI, hence hidden.  pow_build_consts and pow_set_error (pow_template.h) and
// the host-side helpers of include/pow_gpu.h are defined there too.
#pragma once
#include <stdint.h>

#include "../../include/pow_gpu.h"
#include "pow_template.h"

#pragma GCC visibility push(hidden)

// Record a printf-style message for pow_last_error(); returns `code`.
int fail(int code, const char* fmt, ...);
// CLOCK_MONOTONIC in ns: the clock of every deadline in the library.
uint64_t mono_ns();

uint32_t be32(const uint8_t* p);
// block.cpp:79-88 + picosha2.h:201-218: the padded 320-byte message.
void padded_message(const pow_block* b, uint8_t m[320]);
// The argument of K2' (pow_hash_one): the five chunks' K[i] + W[i] words of
// b's padded message.
void pow_build_msg(const pow_block* b, PowMsg* M);
// picosha2's output_hex (picosha2.h:141-150): big-endian digest bytes
// (`digest`, may be null) and lowercase hex + NUL (`hex`, may be null).
void digest_out(const uint32_t* h, uint8_t* digest, char* hex);

// The argument checks shared by the sweep and mine calls.
int check_range(const pow_block* tmpl, uint64_t start, uint64_t count, unsigned diff);
// Split [start, start+count) (count <= 2^32) into K1's prefix form.
int make_launch(uint64_t start, uint64_t count, unsigned diff, uint32_t cap, uint32_t mode, PowLaunch* L);
// K1''s form of [start, start+count): digits, count, diff and thr; the rest
// of *L is zeroed (watch, nwg and seq are the caller's).
void make_launch_lat(uint64_t start, uint64_t count, unsigned diff, PowLaunchLat* L);

// The plan of pow_mine_race's fused path (K6, one launch per height): the
// workgroups a rival gets and the heights queued per batch.  Pure: its inputs
// are the difficulty (<= 32), the rivals (1..256), the window (1..2^32) and the
// chip's CUs, and the test library's two overrides (lanes_log2: 2 is the
// shipped value; batch_override: 0 = none).  It holds that nwg_r >= 1, nwg_r x
// n_rivals <= max(n_rivals, cu_count), 1 <= batch <= 64, and batch x n_rivals x
// ctr_count <= 2^38 whenever batch > 1.
struct PowRacePlan {
  uint32_t nwg_r;  // workgroups per rival
  uint32_t batch;  // heights per batch
};
void pow_race_plan(unsigned diff, uint32_t n_rivals, uint64_t ctr_count, uint32_t cu_count, unsigned lanes_log2,
                   unsigned batch_override, PowRacePlan* p);

// The limits of the two plans below (their kernels are described in pow_ctx.h).
#define POW_CHAIN_MAX_BATCH 64         // K4: launches queued without a host wait
#define POW_BATCH_MAX_TILE (1u << 14)  // K5: templates per launch
#define POW_BATCH_MAX_WG (1u << 16)    // K5: workgroups per launch

// The plan of pow_mine_chain's fused path (K4, one launch per block): the
// launch's workgroups and the blocks queued per batch.  Pure, as the race's:
// the difficulty (<= 32), the window (1..2^32), the slots the context holds
// (one per CU) and the test library's two overrides (lanes_log2: 2 is the
// shipped value; batch_override: 0 = none).  It holds that 1 <= nwg <= max(1,
// grid_max), (nwg - 1) x 256 < ctr_count (no workgroup starts past the window)
// and 1 <= batch <= POW_CHAIN_MAX_BATCH.
struct PowChainPlan {
  uint32_t nwg;    // workgroups per launch
  uint32_t batch;  // blocks per batch
};
PowChainPlan pow_chain_plan(unsigned diff, uint64_t ctr_count, uint32_t grid_max, unsigned lanes_log2,
                            unsigned batch_override);

// The plan of pow_mine_batch's fused path (K5, one launch per tile of the n
// templates): the workgroups a template gets and the templates per launch.
// Pure; lanes_log2 = -1 is the shipped plan (2 down to 0, while the launch
// would exceed one workgroup per CU), tile_override 0 = none.  It holds that 1
// <= nwg_t <= max(1, cu_count), 1 <= tile <= POW_BATCH_MAX_TILE, tile x nwg_t
// <= POW_BATCH_MAX_WG, and tile x ctr_count <= 2^38 whenever tile > 1: an
// override is capped by the window and the workgroups like the planned tile.
struct PowBatchPlan {
  uint32_t nwg_t;  // workgroups per template
  uint32_t tile;   // templates per launch
};
PowBatchPlan pow_batch_plan(unsigned diff, uint64_t n, uint64_t ctr_count, uint32_t cu_count, int lanes_log2,
                            unsigned tile_override);

// ---- the reference's nonce stream (pow_rand_nonces, pow_mine_rand, K8) ----
// glibc's TYPE_3 rand(): r[i] = r[i-31] + r[i-3] over Z/2^32, draw k = r[k +
// 344] >> 1.  The state at draw q is x[0..30] = r[q + 313 .. q + 343]: draw q is
// (x[0] + x[28]) >> 1, which becomes the new x[30].  Moving a state n draws is
// a multiplication by x^n mod (x^31 - x^28 - 1), a polynomial of 31 words.
// None of this calls rand() or srand(): no process-global state.
#define POW_RAND_WORDS 31
// The state at draw 0 of srand(seed) (seed 0 counts as 1).
void pow_rand_seed(uint32_t seed, uint32_t x[POW_RAND_WORDS]);
// The next draw of the state, which moves on by one.
uint32_t pow_rand_draw(uint32_t x[POW_RAND_WORDS]);
// out = a * b mod (x^31 - x^28 - 1); out may be a or b.
void pow_rand_mul(const uint32_t a[POW_RAND_WORDS], const uint32_t b[POW_RAND_WORDS], uint32_t out[POW_RAND_WORDS]);
// c = x^n, by square and multiply.
void pow_rand_power(uint64_t n, uint32_t c[POW_RAND_WORDS]);
// y = the state x moved by the polynomial c: y[j] = sum c[i] * x[i + j] over x
// extended to 61 words by the recurrence.  y may be x.
void pow_rand_apply(const uint32_t c[POW_RAND_WORDS], const uint32_t x[POW_RAND_WORDS], uint32_t y[POW_RAND_WORDS]);
// The nine characters + NUL of the trial the state stands at (9 draws).
void pow_rand_nonce(uint32_t x[POW_RAND_WORDS], char nonce[POW_NONCE_SIZE]);

// The plan of pow_mine_rand (K8, launches of at most 2^26 trials): the trials
// per launch, the launch's workgroups and the run T of consecutive trials a
// lane walks before it jumps to its next run.  Pure: the difficulty (<= 32),
// the window (1..2^32), the chip's CUs and the test library's three overrides
// (lanes_log2: the grid's lanes as a power of two, -1 = the plan: K4's grid;
// run_override: 0 = the plan; launch_log2: 26 is the shipped value).  It holds
// that 1 <= launch <= 2^26, 1 <= nwg <= min(max(1, cu_count), POW_RAND_MAX_WG),
// (nwg - 1) x 256 < min(launch, trial_count), run is a power of two (an
// override: rounded down to one) and 1 <= run <= POW_RAND_MAX_RUN, so a pass
// of the grid is at most 2^26 trials.
#define POW_RAND_MAX_WG 256u
#define POW_RAND_MAX_RUN 1024u
struct PowRandPlan {
  uint64_t launch;  // trials per launch
  uint32_t nwg;     // workgroups per launch
  uint32_t run;     // T
};
PowRandPlan pow_rand_plan(unsigned diff, uint64_t trial_count, uint32_t cu_count, int lanes_log2, unsigned run_override,
                          unsigned launch_log2);
// The two tables of a run T that K8's lanes start from: A[i * 256 + l] = word i
// of x^(9 T l), l < 256 (word-major: a wave reads a word of its 64 lanes'
// polynomials in one line), then B[w * 31 + i] = word i of x^(9 T 256 w), w <
// POW_RAND_MAX_WG.  tab holds POW_RAND_TAB_WORDS words.
#define POW_RAND_TAB_WORDS (POW_RAND_WORDS * 256u + POW_RAND_MAX_WG * POW_RAND_WORDS)
void pow_rand_tables(uint32_t run, uint32_t* tab);
// The three polynomials of a call of K8 or K9: step = x^(9 run (nwg 256 - 1)), from the end of a
// lane's run to its next; first = x^(9 trial_start), to the call's first trial; to_next = x^(9
// per_launch), from a launch's first trial to the next launch's.
void pow_rand_jumps(uint32_t run, uint32_t nwg, uint64_t trial_start, uint64_t per_launch, uint32_t step[POW_RAND_WORDS],
                    uint32_t first[POW_RAND_WORDS], uint32_t to_next[POW_RAND_WORDS]);
// The digit of a character of block.cpp:61-72's alphabet (a-z, A-Z, 0-9 are 0..61), -1 of any other.
int digit_of(char c);

// ---- pow_find_seed (K9): the inverse of pow_rand_nonces ----
// A target's nine base-62 digits as the kernel compares them: w[0] = digits
// 0..4 and w[1] = digits 5..8, six bits each, the first digit highest.
// false, with w not written: a character outside a-z, A-Z, 0-9 in nonce[0..8].
bool pow_seed_pack(const char* nonce, uint32_t w[2]);
// The plan of pow_find_seed: the request's n_seeds x trial_count pairs are cut
// into tiles of `tile` seeds and slices of `slice` trials, one launch per (tile,
// slice) with `nwg` workgroups per seed whose lanes walk runs of `run` trials.
// Pure: the chip's CU count and the test library's overrides (run_override,
// wg_override: 0 = the plan; launch_log2: POW_SEED_LAUNCH_LOG2 is the shipped
// value).  It holds that 1 <= nwg <= POW_RAND_MAX_WG (table B), run = 31 x 2^j
// with j <= 5 (an override: rounded down to one, at least 31), tile x nwg <=
// 2^16 workgroups, 1 <= slice <= 2^26 and nwg x 256 x run <= 2^26 (a lane's
// relative trial stays below 2^27) and tile x slice <= 2^launch_log2 pairs.
#define POW_SEED_LAUNCH_LOG2 30u
struct PowSeedPlan {
  uint32_t tile;   // seeds per launch
  uint32_t nwg;    // workgroups per seed
  uint32_t run;    // T
  uint64_t slice;  // trials per launch
};
PowSeedPlan pow_seed_plan(uint32_t n_seeds, uint64_t trial_count, uint32_t cu_count, unsigned run_override,
                          unsigned wg_override, unsigned launch_log2);

// ---- pow_index_blocks (K10): a pool's block tree ----
// The plan of a pool of n blocks (1..POW_POOL_MAX_BLOCKS): the table's slots,
// the ranking's rounds, and where each array lies in the call's one device
// buffer, in 32-bit words from its start.  Pure; slots_log2 is the test
// library's override (0 = the plan).  It holds that slots is a power of two,
// slots >= 2 n (an override: 2^slots_log2, raised to the lowest power of two
// that is at least n + 1, so that a probe always meets an empty slot), rounds =
// ceil(log2 n) (2^rounds >= n: the deepest walk of n blocks has ended), no two
// arrays overlap, dig and prev lie on 16 bytes and ctl on 8, and words holds
// them all: 4 + 24 n + 2 ceil(n / 4) + slots, that is 98 bytes per block and 4
// per slot (8 to 16 per block): 111 MB at 2^20 blocks.
struct PowPoolPlan {
  uint32_t slots;     // of the table
  uint32_t rounds;    // of pointer jumping
  uint32_t ctl;       // PowPoolCtl: 4 words
  uint32_t dig;       // 8 n: the computed digests
  uint32_t prev;      // 8 n: the parsed previous_block_hash
  uint32_t index;     // n
  uint32_t parent;    // n
  uint32_t next[2];   // n each: the ranking's ping-pong buffers ...
  uint32_t depth[2];
  uint32_t bad[2];
  uint32_t status;    // n bytes
  uint32_t kind;      // n bytes
  uint32_t table;     // slots
  uint64_t words;     // all of it
};
PowPoolPlan pow_pool_plan(uint32_t n, unsigned slots_log2);

// ---- pow_pool (K11): the pool that stays on the device ----
// The plan of a pool's arrays at a capacity of cap blocks (1..
// POW_POOL_MAX_BLOCKS): K10's arrays at cap entries each, in 32-bit words from
// the start of the pool's buffer; the table is an allocation of its own.  Pure.
// It holds that no two arrays overlap, dig and prev lie on 16 bytes, ctl on 8,
// status and kind on whole words, and words holds them all: 8 + 24 cap +
// 2 ceil(cap / 4), that is 98 bytes per block as pow_index_blocks has them.
#define POW_POOL_LIVE_CTL_WORDS 6u   // PowPoolLiveCtl (pow_ctx.h); the plan rounds them up to 8
#define POW_POOL_LIVE_FIRST_CAP 64u  // pow_pool_open with reserve 0: 1,024 blocks take four doublings
struct PowPoolLivePlan {
  uint32_t cap;       // blocks the arrays hold
  uint32_t ctl;       // PowPoolLiveCtl
  uint32_t dig, prev, index, parent, next[2], depth[2], bad[2];  // as PowPoolPlan's, cap entries each
  uint32_t status, kind;  // cap bytes each
  uint64_t words;
};
PowPoolLivePlan pow_pool_live_plan(uint32_t cap);
// The first capacity: reserve, or with reserve 0 POW_POOL_LIVE_FIRST_CAP
// (first_cap: the test library's override of that, 0 = none); 1..POW_POOL_MAX_BLOCKS.
uint32_t pow_pool_live_first_cap(size_t reserve, unsigned first_cap);
// The capacity for `need` blocks (cap < need <= POW_POOL_MAX_BLOCKS): cap
// doubled until it holds them, never past POW_POOL_MAX_BLOCKS.
uint32_t pow_pool_live_grow(uint32_t cap, uint32_t need);
// The first table: the lowest power of two that is at least 2 cap, or the test
// library's 2^slots_log2 (2..2^21; 0 = none).
uint32_t pow_pool_live_first_slots(uint32_t cap, unsigned slots_log2);
// The table for `size` blocks after an add: `slots` if size <= slots / 2,
// otherwise (a rebuild) the lowest power of two that is at least 2 size.  So
// slots >= 2 size after every add, and a probe always meets an empty slot.
uint32_t pow_pool_live_slots(uint32_t slots, uint32_t size);
// ceil(log2 n), 0 for n <= 1: the rounds that end every walk of n blocks; pow_pool_plan's rounds.
uint32_t pow_pool_rounds(uint32_t n);
// The kernel launches of an add of m blocks (m >= 1) that leaves `size` blocks:
// one K10a per host tile of 2^16, the insert (K11b, or K10b on a rebuild), K11c,
// ceil(log2 m) rounds of K11d and K11e: what pow_index_blocks takes on the m
// blocks alone.  A re-rank adds K11s, K10c, ceil(log2 size) rounds of K10d and K10e.
uint32_t pow_pool_live_launches(uint32_t m, uint32_t size, bool rerank);

// ---- pow_pool_mark, pow_pool_prune (K12) ----
// The capacity a prune leaves for `kept` blocks (0..POW_POOL_MAX_BLOCKS): the lowest
// power of two that holds them and is at least first_cap, what pow_pool_open takes
// with reserve 0 (pow_pool_live_first_cap(0, ...)); at least 1, never past
// POW_POOL_MAX_BLOCKS.  The table beside it is pow_pool_live_slots(
// pow_pool_live_first_slots(cap, slots_log2), kept): slots >= 2 kept, as after an add.
uint32_t pow_pool_prune_cap(uint32_t kept, uint32_t first_cap);
uint32_t pow_pool_prune_slots(uint32_t cap, uint32_t kept, unsigned slots_log2);
// The kernel launches of a mark (prune = false) or a prune of a pool of `size`
// blocks of which `kept` are marked: K12a, ceil(log2 size) rounds of K12b, K12c
// and K12d; a prune that drops some blocks and keeps some adds K12e, K12f and
// K10b.  An empty pool: 0.
uint32_t pow_pool_prune_launches(uint32_t size, uint32_t kept, bool prune);

// ---- pow_pool_ancestors, pow_pool_fork_points, pow_pool_chain (K13) ----
// The binary-lifting table of a pool of n blocks: its level 0 is the pool's
// parent array, and it has max(pow_pool_rounds(n) - 1, 0) rows of its own.
uint32_t pow_pool_lift_rows(uint32_t n);
// The device memory of a table made at a capacity of cap blocks: 4 cap rows(cap) bytes.
uint64_t pow_pool_lift_bytes(uint32_t cap);
// The launches that bring a table that covers `covered` blocks up to a pool of
// `size` (covered <= size).  stale: it is made from nothing, one launch per
// row.  Otherwise, for the m = size - covered new blocks, the rows that exist:
// one launch of one workgroup when m <= POW_POOL_LIFT_SMALL, else one per row;
// then one launch for every row that is new because size passed a power of two.
#define POW_POOL_LIFT_SMALL 256u
uint32_t pow_pool_lift_launches(uint32_t covered, uint32_t size, bool stale);

#pragma GCC visibility pop
