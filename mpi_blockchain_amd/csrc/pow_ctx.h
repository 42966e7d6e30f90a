// The context of the C ABI, the holders of its grow-on-demand buffers and what
// pow_api.cpp shares with the test library's hooks (pow_hooks.cpp).  Private to
// csrc/; not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <string>

#include "pow_host.h"
#include "pow_lift_dev.h"

#define HIP_OK(expr)                                                                       \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess)                                                                  \
      return fail(POW_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, \
                  __LINE__);                                                               \
  } while (0)

struct pow_aql;  // the direct dispatcher (pow_aql.h): test library only

// The context's buffers that are made at the first call that needs them, or
// grow with a call's size: a pointer and its capacity in elements, in device
// memory (DevBuf) or pinned host memory (HostBuf).  reserve(n) keeps what it
// has when n <= cap; otherwise it frees first and allocates after, so a grown
// buffer never stands beside its predecessor.  No destructor frees them:
// pow_destroy leaves a wedged context's memory allocated under a kernel that
// may still write it, and that stays its explicit decision
// (pow_ctx::release_buffers, which has to name every holder of pow_ctx: one
// that is added and not listed there leaks).  A failed allocation is reported
// with the buffer's name (`what`; RESERVE passes the expression).
template <class T, bool kPinned>
struct CtxBuf {
  T* p = nullptr;
  size_t cap = 0;
  void release() {
    if (p) (void)(kPinned ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    cap = 0;
  }
  int reserve(size_t n, const char* what) {
    if (n <= cap) return POW_OK;
    release();
    const hipError_t e = kPinned ? hipHostMalloc(&p, n * sizeof(T), hipHostMallocDefault) : hipMalloc(&p, n * sizeof(T));
    if (e != hipSuccess)
      return fail(POW_EHIP, "%s of %s (%zu bytes) failed: %s", kPinned ? "hipHostMalloc" : "hipMalloc", what,
                  n * sizeof(T), hipGetErrorString(e));
    cap = n;
    return POW_OK;
  }
};
#define RESERVE(buf, n)                                   \
  do {                                                    \
    if (int rc_ = (buf).reserve((n), #buf)) return rc_;   \
  } while (0)
template <class T> using DevBuf = CtxBuf<T, false>;
template <class T> using HostBuf = CtxBuf<T, true>;

// Result words of K3 (pow_verify_kernel): reset by the host before a launch.
struct PowVerifyRes {
  unsigned int first_bad;  // lowest flagged block of the launch (atomic min); ~0 = none
  unsigned int n_bad;      // flagged blocks (atomic add)
};

// K7 (pow_verify_batch_kernel, pow_verify_batch.hip), one launch per host tile
// of pow_verify_chains: its verdict is two words per chain, first_bad (atomic
// min of the position within the chain; ~0 = none) and n_bad (atomic add),
// reset by the host before the call's first launch.

// What K4, K5 and K6 share (pow_walk_dev.h: the lowest-key search and the seal).
// The workgroups that count themselves out on one exit word: the word counts
// them in its low 16 bits and carries their trials (at most 2^40 + one per
// lane) above.  Every launch wrapper refuses a larger count.
#define POW_WALK_MAX_WG (1u << 16)
// The head of every launch's arguments: the window and the threshold.
struct PowWalkHead {
  uint32_t base_digit[9];  // base-62 digits of ctr_start (nonce[0..8])
  uint32_t thr;            // a digest solves iff H0 <= thr (d <= 32)
  uint64_t count;          // counters [ctr_start, ctr_start + count), count <= 2^32
};
// One workgroup's lowest hit of a launch, written before it leaves (rel = ~0:
// none).  rel holds the search's key: K4, K5 the relative counter, K6 the race's key.
struct PowChainSlot {
  unsigned long long rel;
  unsigned int digest[8];
};
// Control words of a batch of K4 or K6 launches: reset by the host before the
// batch; min_key and exits are reset again by each launch's sealing workgroup
// for the next one.
struct PowSealCtl {
  // lowest solving key of the running launch (atomic min); ~0 = none.  K4: counter - ctr_start;
  // K6: (counter - ctr_start) << 8 | rival
  unsigned long long min_key;
  unsigned long long hashes;   // trials computed, all launches of the batch (added by each launch's sealer)
  unsigned long long exits;    // the running launch: workgroups that have left (low 16 bits), their trials above
  unsigned int stop;           // a launch in which no window held a solution: every later launch exits at once
  unsigned int n_done;         // blocks sealed by the batch
};

// K4 (pow_chain_kernel, pow_chain.hip), one launch per block of pow_mine_chain,
// at most POW_CHAIN_MAX_BATCH (pow_host.h) queued without a host wait.
// pow_mine_chain: above it the host loop over pow_mine.  The largest measured d
// at which the fused call beat the host loop (profiles/mine_chain/README.md).
#define POW_CHAIN_FUSED_MAX_D 23
// A batch in device memory, and its pinned twin: parent and ctl go up in one
// copy, ctl and the sealed blocks come down in one.  Block j of the batch is
// blk[nb - 1 - j] (tip first); its launch reads blk[nb - j], the first parent.
struct PowChainBuf {
  pow_block parent;
  PowSealCtl ctl;
  pow_block blk[POW_CHAIN_MAX_BATCH];
};
// The arguments of one launch.
struct PowChainLaunch {
  PowWalkHead w;
  uint32_t owner, diff;    // the template's node_owner_number and difficulty
  uint32_t nwg;            // workgroups of the launch (= gridDim.x)
  uint32_t pad;
  uint64_t created_at;     // the template's created_at
};

// K5 (pow_batch_kernel, pow_batch.hip), one launch per tile of pow_mine_batch's
// templates: POW_BATCH_MAX_TILE templates and POW_BATCH_MAX_WG workgroups at most (pow_host.h).
static_assert(POW_BATCH_MAX_WG <= POW_WALK_MAX_WG, "a template's workgroups fit the exit word's count");
// pow_mine_batch: above it the host loop over pow_mine.  The largest measured d
// at which the fused call beat the C loop at n = 64 by more than the two
// interquartile ranges combined (profiles/mine_batch/README.md); -1 = nowhere.
#define POW_BATCH_FUSED_MAX_D 23
// Control words of one template of a tile: reset by the host before the launch.
struct PowBatchCtl {
  unsigned long long min_rel;  // lowest solving (counter - ctr_start) of the template (atomic min); ~0 = none
  unsigned long long exits;    // the template's workgroups that have left (low 16 bits), their trials above
};
// One template's result, written by the last of its workgroups to leave.
struct PowBatchRec {
  unsigned long long rel;  // lowest solving (counter - ctr_start); ~0 = the window holds none
  unsigned int digest[8];  // its digest
  unsigned long long trials;
};
// The arguments of a launch: the tile's templates share window and difficulty.
struct PowBatchLaunch {
  PowWalkHead w;
  uint32_t nwg_t;          // workgroups per template; gridDim.x = nwg_t x the tile's templates
  uint32_t pad;
};

// K6 (pow_race_kernel, pow_race.hip), one launch per height of pow_mine_race.
#define POW_RACE_MAX_BATCH 64       // launches queued without a host wait
#define POW_RACE_MAX_WG POW_WALK_MAX_WG  // a launch stays below it: every workgroup counts out on one exit word
// pow_mine_race: above it the host loop over pow_mine.  The largest measured d
// at which the fused call beat the host loop at 3 and at 64 rivals by more than
// the two interquartile ranges combined (profiles/mine_race/README.md); -1 = nowhere.
#define POW_RACE_FUSED_MAX_D 23
// One height's result, written by the launch's sealing workgroup.
struct PowRaceRec {
  unsigned long long rel;  // the winner's (counter - ctr_start)
  unsigned int winner;     // its position in owners[]
  unsigned int pad;
};
// A batch in device memory, and its pinned twin: parent and ctl go up in one
// copy; ctl, the records and the sealed blocks come down in one.  Height j of
// the batch is rec[j] and blk[nb - 1 - j] (tip first); its launch reads
// blk[nb - j], the first parent.
struct PowRaceBuf {
  pow_block parent;
  PowSealCtl ctl;
  PowRaceRec rec[POW_RACE_MAX_BATCH];
  pow_block blk[POW_RACE_MAX_BATCH];
};
// What the rivals differ in, as it goes up once per batch: rival r of the
// batch's height j has owner[r] and created_at[j * n_rivals + r].
struct PowRaceIn {
  uint32_t owner[POW_RACE_MAX_RIVALS];
  uint64_t created_at[POW_RACE_MAX_BATCH * POW_RACE_MAX_RIVALS];
};
// The arguments of one launch.
struct PowRaceLaunch {
  PowWalkHead w;
  uint32_t diff;           // the templates' difficulty
  uint32_t n_rivals;       // 1..256
  uint32_t nwg_r;          // workgroups per rival; gridDim.x = nwg_r x n_rivals
  uint32_t height;         // of the batch: the row of PowRaceIn::created_at, and the record to write
};

// K8 (pow_rand_kernel, pow_rand.hip), one launch per 2^26 trials at most of
// pow_mine_rand: the search of K4-K6 over the nonces of the reference's rand()
// stream.  What goes up per launch, in one copy:
struct PowRandIn {
  PowBatchCtl ctl;                  // min_rel = the lowest solving trial relative to the launch; reset by the host
  uint32_t state[POW_RAND_WORDS];   // the generator's state at the launch's first trial
  uint32_t thr;                     // a digest solves iff H0 <= thr
  uint32_t step[POW_RAND_WORDS];    // x^(9 T (G - 1)): from the end of a lane's run to its next
  uint32_t pad;
  pow_block tmpl;                   // the raw struct, hashed as it stands (as K5)
};
static_assert(offsetof(PowRandIn, tmpl) % 4 == 0 && sizeof(PowRandIn) % 8 == 0, "dwords");
// ... and what comes down: written by the last workgroup to leave.
struct PowRandRec {
  unsigned long long rel;     // lowest solving trial relative to the launch; ~0 = the launch holds none
  unsigned int digest[8];     // its digest
  unsigned long long trials;
  unsigned int nonce_w[3];    // message words 1 and 2 and the top byte of word 3 as the winning lane hashed them
  unsigned int pad;
};
// The arguments of a launch.
struct PowRandLaunch {
  uint32_t count;  // trials of the launch, <= 2^26
  uint32_t run;    // T: consecutive trials of a lane per pass, <= POW_RAND_MAX_RUN
  uint32_t nwg;    // workgroups (= gridDim.x), <= POW_RAND_MAX_WG
  uint32_t pad;
};

// K9 (pow_seed_kernel, pow_seed.hip), one launch per (tile of seeds, slice of
// trials) of pow_find_seed: K8's walk without the hash, every seed of the tile
// seeded on the device.  What goes up per launch, in one copy:
struct PowSeedIn {
  uint32_t jump[POW_RAND_WORDS];   // x^(9 x the slice's first trial): from a seed's draw 0 to the launch's start
  uint32_t n_targets;              // 1..POW_SEED_MAX_TARGETS
  uint32_t step[POW_RAND_WORDS];   // x^(9 T (G - 1)): from the end of a lane's run to its next
  uint32_t pad;
  unsigned long long pair[62];     // bit d1 of pair[d0]: some target begins with the digits d0, d1
  unsigned long long pair2[62];    // bit d3 of pair2[d2]: some target has the digits d2, d3 in third and fourth place
  uint32_t tgt[POW_SEED_MAX_TARGETS][2];  // pow_seed_pack of each target
};
static_assert(sizeof(PowSeedIn) % 8 == 0 && offsetof(PowSeedIn, pair) % 8 == 0, "dwords, the table on 8 bytes");
// ... and what comes down: a counter (reset by the host before the launch) and
// the matches in the order their lanes reserved them.  A launch that counts more
// than the list holds fails the call; 64 targets that all occur in one launch
// under seeds 0 and 1 are 128.
#define POW_SEED_DEV_CAP 1024u
struct PowSeedRec {
  uint32_t pos;     // the seed's position in the request
  uint32_t target;  // index into the targets
  uint32_t rel;     // the trial relative to the launch's first
};
struct PowSeedOut {
  uint32_t n;       // matches of the launch (atomic add)
  uint32_t pad;
  PowSeedRec rec[POW_SEED_DEV_CAP];
};
// The arguments of a launch; gridDim.x = n_seeds x nwg.
struct PowSeedLaunch {
  uint32_t seed_first;  // the request's first seed; the seed at position p is seed_first + p mod 2^32
  uint32_t pos_base;    // the position of the tile's first seed
  uint32_t n_seeds;     // seeds of the tile
  uint32_t count;       // trials of the slice, <= 2^26
  uint32_t run;         // T = 31 x 2^j, j <= 5
  uint32_t nwg;         // workgroups per seed, <= POW_RAND_MAX_WG
};

// K10 (pow_pool.hip), the kernels of pow_index_blocks.  What a block's
// previous_block_hash can be (K10a writes it, K10c reads it):
enum { POW_PREV_EMPTY = 0, POW_PREV_DIGEST = 1, POW_PREV_UNMATCHABLE = 2 };
// The call's control words: reset by the host before K10b.
struct PowPoolCtl {
  unsigned int err;         // K10b: a lane found no slot (atomic or)
  unsigned int n_flagged;   // K10e: blocks with a non-zero status (atomic add)
  unsigned long long best;  // K10e: the greatest index << 32 | ~position among n_bad == 0 (atomic max); 0 = none
};
static_assert(sizeof(PowPoolCtl) == 16, "four words of the plan");
// The arrays of a call, each n entries unless said: device addresses in the
// call's one buffer, at the plan's offsets (pow_pool_plan, pow_host.h).
struct PowPoolDev {
  PowPoolCtl* ctl;
  uint32_t* dig;     // 8 n: the computed digests
  uint32_t* prev;    // 8 n: the parsed previous_block_hash
  uint32_t* index;
  uint32_t* parent;
  uint32_t* next[2];
  uint32_t* depth[2];
  uint32_t* bad[2];
  uint8_t* status;
  uint8_t* kind;
  uint32_t* table;   // slots
  uint32_t n, slots;
};
inline PowPoolDev pow_pool_dev(uint32_t* base, const PowPoolPlan& p, uint32_t n) {
  return PowPoolDev{(PowPoolCtl*)(base + p.ctl), base + p.dig, base + p.prev, base + p.index, base + p.parent,
                    {base + p.next[0], base + p.next[1]}, {base + p.depth[0], base + p.depth[1]},
                    {base + p.bad[0], base + p.bad[1]}, (uint8_t*)(base + p.status), (uint8_t*)(base + p.kind),
                    base + p.table, n, p.slots};
}

// K11 (pow_pool_live.hip), the kernels of pow_pool_add and pow_pool_find.  The
// pool's control words stay on the device from add to add: K10's first (K10b
// and K10e take them as they are), then the orphans of the last add whose
// parent came with it, which the host resets before every add.
struct PowPoolLiveCtl {
  PowPoolCtl k10;        // err; n_flagged and best over the whole pool, fed by every add
  unsigned int adopted;  // K11c: old blocks that were POW_POOL_NONE and have a parent now (atomic add)
  unsigned int marked;   // K12d: the blocks the last pow_pool_mark or pow_pool_prune marked; every add resets it
};
static_assert(sizeof(PowPoolLiveCtl) == 4 * POW_POOL_LIVE_CTL_WORDS && offsetof(PowPoolLiveCtl, k10) == 0,
              "the plan's control words; K10's launchers take the head");
// A pool's arrays at its capacity's offsets (pow_pool_live_plan) with its
// table, which is an allocation of its own; n = the blocks it holds.
inline PowPoolDev pow_pool_live_dev(uint32_t* base, const PowPoolLivePlan& p, uint32_t* table, uint32_t n,
                                    uint32_t slots) {
  return PowPoolDev{(PowPoolCtl*)(base + p.ctl), base + p.dig, base + p.prev, base + p.index, base + p.parent,
                    {base + p.next[0], base + p.next[1]}, {base + p.depth[0], base + p.depth[1]},
                    {base + p.bad[0], base + p.bad[1]}, (uint8_t*)(base + p.status), (uint8_t*)(base + p.kind),
                    table, n, slots};
}

// K14 (pow_pool_above.hip): one root's record of pow_pool_subtrees and pow_pool_drop, zeroed by the host before K14d.
struct PowAboveAcc {
  unsigned long long best;  // K10e's key over the members with n_bad == 0 (atomic max); 0 = none
  unsigned int size;        // the members (atomic add)
  unsigned int height;      // the greatest depth over the root's among them (atomic max)
};
static_assert(sizeof(PowAboveAcc) == 16, "four words a root in d_find");

struct pow_ctx {
  int device = 0;
  int cu_count = 0;
  int clock_khz = 0;
  int realtime_khz = 100000;  // s_memrealtime rate (hipDeviceAttributeWallClockRate)
  uint32_t lat_seq = 0;       // K1' launches so far (PowLaunchLat::seq)
  PowConstsLat lat_consts{};  // K1''s kernel argument (the subset of h_blob->consts it reads)
  char name[256] = {0};
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipEvent_t ev_block = nullptr;  // polled with sleeps during long launches
  PowBlob* d_blob = nullptr;   // per-template constants + result words, one allocation
  PowBlob* h_blob = nullptr;   // pinned staging copy: uploaded with one H2D per launch
  bool consts_dirty = false;   // h_blob->consts not yet on the device
  PowResult* d_lat = nullptr;           // latency kernel: self-resetting device result words ...
  PowResult* h_lat = nullptr;           // ... published by its last wave here (mapped host memory)
  PowHashOut* h_one = nullptr;          // K2' (pow_hash_block): digest + done word (mapped host memory)
  PowHashOut* d_one = nullptr;          // device address of h_one
  uint32_t one_seq = 0;                 // K2' launches so far (the done word's value)
  PowResult* d_lat_host = nullptr;      // device address of h_lat
  unsigned int* h_epoch = nullptr;      // pow_cancel's word: mapped, coherent host memory ...
  unsigned int* d_epoch = nullptr;      // ... and its device address
  std::atomic<bool> armed{false};       // pow_cancel has published an epoch
  uint32_t launch_epoch = 0;            // mine calls: the caller's epoch ...
  bool watch_epoch = false;             // ... watched on the GPU when armed
  pow_board* board = nullptr;           // bound stop board (pow_board_bind) ...
  const unsigned long long* board_dev = nullptr;  // ... its slots, device address
  int board_slot = -1;
  uint32_t board_tag = 0;
  bool board_off = false;               // winner re-hash: not part of the search
  PowConsts* d_consts = nullptr;  // = &d_blob->consts
  PowResult* d_res = nullptr;     // = &d_blob->res
  PowResult* h_res = nullptr;  // pinned read-back of d_res
  uint32_t* d_tail = nullptr;  // sweep: per-wave remainders (< 32 each), appended after the launch
  uint32_t tail_cap = 0;
  // Made or grown by the call that needs them (release_buffers frees them):
  DevBuf<uint32_t> d_out, d_alt;     // pow_sweep's device list and its radix-sort twin ...
  DevBuf<uint8_t> d_sort_tmp;        // ... and the sort's scratch, in bytes
  DevBuf<uint32_t> d_msgs, d_dig;    // pow_hash_blocks: 80 message words in, 8 digest words out per block
  DevBuf<pow_block> d_vblk;          // pow_verify_chain[s]: one host tile of raw structs + its halo block,
  DevBuf<uint8_t> d_vstatus;         // the tile's status bytes
  DevBuf<PowVerifyRes> d_vres;       // K3's result words ...
  HostBuf<PowVerifyRes> h_vres;      // ... and their pinned twin: reset value up, result down
  DevBuf<uint32_t> d_voffs;          // pow_verify_chains: the chains' offsets (n_chains + 1 words) ...
  DevBuf<uint32_t> d_vcres;          // ... K7's verdicts: first_bad, then n_bad, a call's n_chains words each ...
  HostBuf<uint32_t> h_vchains;       // ... and the pinned twin of both: the offsets up, the verdicts down
  DevBuf<PowChainBuf> d_chain;       // pow_mine_chain: a batch on the device ...
  HostBuf<PowChainBuf> h_chain;      // ... its pinned twin ...
  DevBuf<PowChainSlot> d_cslot;      // ... and one slot per workgroup of the largest K4 launch: one per CU
  DevBuf<uint8_t> d_batch;           // pow_mine_batch: a tile's control words, then its raw structs ...
  HostBuf<uint8_t> h_batch;          // ... and the pinned twin they go up from in one copy
  DevBuf<PowBatchRec> d_brec;        // the tile's result records ...
  HostBuf<PowBatchRec> h_brec;       // ... and their pinned twin
  DevBuf<PowChainSlot> d_bslot;      // one slot per workgroup of a K5 launch (POW_BATCH_MAX_WG)
  DevBuf<PowRaceBuf> d_race;         // pow_mine_race: a batch on the device ...
  HostBuf<PowRaceBuf> h_race;        // ... its pinned twin ...
  DevBuf<PowRaceIn> d_rin;           // ... the rivals' owners and created_at ...
  HostBuf<PowRaceIn> h_rin;          // ... and the pinned twin they go up from
  DevBuf<PowChainSlot> d_rslot;      // one slot per workgroup of a K6 launch: max(POW_RACE_MAX_RIVALS, cu_count)
  DevBuf<PowRandIn> d_rand;          // pow_mine_rand: a launch's input on the device ...
  HostBuf<PowRandIn> h_rand;         // ... and its pinned twin
  DevBuf<PowRandRec> d_rrec;         // the launch's record ...
  HostBuf<PowRandRec> h_rrec;        // ... and its pinned twin
  DevBuf<PowChainSlot> d_rnslot;     // one slot per workgroup of a K8 launch (POW_RAND_MAX_WG) ...
  DevBuf<uint32_t> d_rnchar;         // ... and the three nonce words of its hit
  DevBuf<uint32_t> d_rtab;           // the two tables of the run T below (pow_rand_tables) ...
  HostBuf<uint32_t> h_rtab;          // ... and the pinned twin they go up from
  uint32_t rand_tab_run = 0;         // the T the tables on the device were made for (0 = none yet)
  DevBuf<PowSeedIn> d_seed;          // pow_find_seed: a launch's input on the device ...
  HostBuf<PowSeedIn> h_seed;         // ... and its pinned twin
  DevBuf<PowSeedOut> d_sout;         // the launch's matches ...
  HostBuf<PowSeedOut> h_sout;        // ... and their pinned twin (d_rtab, h_rtab: K9 starts from K8's tables)
  DevBuf<uint32_t> d_pool;           // pow_index_blocks: every array of the call (pow_pool_plan), in words ...
  HostBuf<PowPoolCtl> h_pool;        // ... and the pinned twin of its control words
  void release_buffers() {  // every holder above
    d_pool.release(), h_pool.release();
    d_seed.release(), h_seed.release(), d_sout.release(), h_sout.release();
    d_rand.release(), h_rand.release(), d_rrec.release(), h_rrec.release();
    d_rnslot.release(), d_rnchar.release(), d_rtab.release(), h_rtab.release();
    d_out.release(), d_alt.release(), d_sort_tmp.release();
    d_msgs.release(), d_dig.release();
    d_vblk.release(), d_vstatus.release(), d_vres.release(), h_vres.release();
    d_voffs.release(), d_vcres.release(), h_vchains.release();
    d_chain.release(), d_cslot.release(), h_chain.release();
    d_batch.release(), d_brec.release(), d_bslot.release(), h_batch.release(), h_brec.release();
    d_race.release(), d_rin.release(), d_rslot.release(), h_race.release(), h_rin.release();
  }
  unsigned grid_full = 0;  // workgroups that fill the chip (8 per CU)
  // Set only by the test library's hooks (pow_hooks.cpp, at pow_init):
  bool force_full = false;        // use the d > 32 kernel for every d
  const char* fault_mine = nullptr;  // non-null: every pow_mine[_any] call fails with this text (failure-propagation tests)
  uint64_t lat_max = 1ull << 24;  // first-sub-round cap for K1' (0 = K1 only)
  unsigned lat_wps = 0;           // K1' waves per SIMD at every d (0 = the plan)
  bool sentinel_idle = false;     // K1 mine launches: the sentinel wave takes no chunk (POW_LAUNCH_SENTINEL_IDLE)
  unsigned test_stall_us = 0;     // a bounded stall kernel in front of every HIP launch (watchdog tests)
  unsigned chain_batch = 0;       // pow_mine_chain: blocks per batch (0 = the plan)
  unsigned chain_lanes_log2 = 2;  // K4's grid: lanes = 2^this x the expected 2^d trials
  int chain_fused_max = POW_CHAIN_FUSED_MAX_D;  // pow_mine_chain: highest d on the fused path (-1 = host loop only)
  unsigned batch_tile = 0;        // pow_mine_batch: templates per launch (0 = the plan)
  int batch_lanes_log2 = -1;      // K5's lanes per template = 2^this x the expected 2^d trials (-1 = the plan: 2 down to 0)
  int batch_fused_max = POW_BATCH_FUSED_MAX_D;  // pow_mine_batch: highest d on the fused path (-1 = host loop only)
  unsigned race_batch = 0;        // pow_mine_race: heights per batch (0 = the plan)
  unsigned race_lanes_log2 = 2;   // K6's grid: lanes over all rivals = 2^this x the expected 2^d trials
  int race_fused_max = POW_RACE_FUSED_MAX_D;  // pow_mine_race: highest d on the fused path (-1 = host loop only)
  unsigned rand_run = 0;          // pow_mine_rand: K8's run T (0 = the plan)
  int rand_lanes_log2 = -1;       // K8's grid: 2^this lanes (-1 = the plan: K4's grid)
  unsigned rand_launch_log2 = 26; // trials per K8 launch = 2^this
  unsigned seed_run = 0;          // pow_find_seed: K9's run T (0 = the plan)
  unsigned seed_wg = 0;           // K9's workgroups per seed (0 = the plan)
  unsigned seed_launch_log2 = POW_SEED_LAUNCH_LOG2;  // (seed, trial) pairs per K9 launch = 2^this
  unsigned pool_slots_log2 = 0;   // pow_index_blocks: the table's slots = 2^this, at least n + 1 (0 = the plan);
                                  // pow_pool_open: the pool's first table
  unsigned pool_first_cap = 0;    // pow_pool_open with reserve 0: the first capacity in blocks (0 = the plan)
  unsigned open_pools = 0;        // pow_pool handles not yet closed: pow_destroy keeps the context while there are any
  // K1' and K2' launches as AQL packets (pow_aql.cpp) instead of
  // hipLaunchKernel: test library only, opt-in there; null = the HIP launch
  // path, the only one the shipped library has.
  pow_aql* aql = nullptr;
  std::string aql_why;            // why aql is null, if it is
  // Watchdog (every host wait on a launch is bounded): base deadline of a
  // latency launch, and of a throughput launch on top of its per-counter share.
  uint64_t watchdog_ns = 10ull * 1000000000ull;
  // A watchdog fired (or a direct dispatch was refused after its packet slot
  // was reserved): a launch of this context may still be queued.  pow_group_*
  // then do not queue a collective behind it; pow_destroy frees only what a
  // bounded wait shows drained.
  bool wedged = false;
  bool aql_lost = false;  // the direct dispatcher was closed with a packet still in flight
  pow_stats stats{};
};

// The launch wrappers of the .hip files.
hipError_t pow_launch_search(int mode, bool full, unsigned grid, hipStream_t stream, const PowConsts* C,
                             const PowLaunch& L, uint32_t* out, PowResult* res);
hipError_t pow_launch_hash(uint32_t n, hipStream_t stream, const uint32_t* msgs, uint32_t* digests);
hipError_t pow_launch_hash_one(hipStream_t stream, const PowMsg& M, PowHashOut* hout, uint32_t seq);
hipError_t pow_launch_verify(uint32_t n_check, uint32_t n_avail, unsigned diff, hipStream_t stream,
                             const uint32_t* blocks, uint8_t* status, PowVerifyRes* res);
hipError_t pow_launch_verify_batch(uint32_t n_check, uint32_t n_avail, uint32_t base, unsigned diff,
                                   hipStream_t stream, const uint32_t* blocks, const uint32_t* offs,
                                   uint32_t n_chains, uint8_t* status, uint32_t* first_bad, uint32_t* n_bad);
hipError_t pow_launch_chain(hipStream_t stream, const PowChainLaunch& L, const uint32_t* prev, uint32_t* dst,
                            PowSealCtl* ctl, PowChainSlot* slots);
hipError_t pow_launch_batch(hipStream_t stream, const PowBatchLaunch& L, uint32_t n_tmpl, const uint32_t* tmpls,
                            PowBatchCtl* ctl, PowChainSlot* slots, PowBatchRec* rec);
hipError_t pow_launch_race(hipStream_t stream, const PowRaceLaunch& L, const uint32_t* prev, uint32_t* dst,
                           const PowRaceIn* in, PowSealCtl* ctl, PowChainSlot* slots, PowRaceRec* rec);
hipError_t pow_launch_rand(hipStream_t stream, const PowRandLaunch& L, const PowRandIn* in, const uint32_t* tab,
                           PowBatchCtl* ctl, PowChainSlot* slots, uint32_t* slot_nonce, PowRandRec* rec);
hipError_t pow_launch_seed(hipStream_t stream, const PowSeedLaunch& L, const PowSeedIn* in, const uint32_t* tab,
                           PowSeedOut* out);
hipError_t pow_launch_pool_audit(hipStream_t stream, const uint32_t* blocks, uint32_t n_check, uint32_t base,
                                 unsigned diff, const PowPoolDev& D);
hipError_t pow_launch_pool_insert(hipStream_t stream, const PowPoolDev& D);
hipError_t pow_launch_pool_join(hipStream_t stream, const PowPoolDev& D);
hipError_t pow_launch_pool_round(hipStream_t stream, const PowPoolDev& D, uint32_t r);
hipError_t pow_launch_pool_finish(hipStream_t stream, const PowPoolDev& D, uint32_t which);
hipError_t pow_launch_pool_live_insert(hipStream_t stream, const PowPoolDev& D, uint32_t base);
hipError_t pow_launch_pool_live_join(hipStream_t stream, const PowPoolDev& D, uint32_t base);
hipError_t pow_launch_pool_live_round(hipStream_t stream, const PowPoolDev& D, uint32_t base, uint32_t from);
hipError_t pow_launch_pool_live_finish(hipStream_t stream, const PowPoolDev& D, uint32_t base, uint32_t which,
                                       uint32_t fin);
hipError_t pow_launch_pool_live_strip(hipStream_t stream, const PowPoolDev& D);
hipError_t pow_launch_pool_live_find(hipStream_t stream, const PowPoolDev& D, const uint32_t* names, uint32_t k,
                                     uint32_t* pos);
// K12 (pow_pool_prune.hip), the kernels of pow_pool_mark and pow_pool_prune.  D, F: the pool's arrays; T: the
// arrays a prune gathers into; fin: which of depth[], bad[] hold the final values (the others are scratch).
hipError_t pow_launch_pool_prune_seed(hipStream_t stream, const PowPoolDev& D, uint32_t fin, const uint32_t* tips,
                                      uint32_t n_tips, uint32_t min_index, uint32_t flags);
hipError_t pow_launch_pool_prune_round(hipStream_t stream, const PowPoolDev& D, uint32_t fin, uint32_t r);
hipError_t pow_launch_pool_prune_count(hipStream_t stream, const PowPoolDev& D, uint32_t fin);
hipError_t pow_launch_pool_prune_scan(hipStream_t stream, const PowPoolDev& D);
hipError_t pow_launch_pool_prune_gather(hipStream_t stream, const PowPoolDev& F, const PowPoolDev& T, uint32_t cap,
                                        uint32_t fin);
hipError_t pow_launch_pool_prune_remap(hipStream_t stream, const PowPoolDev& F, const PowPoolDev& T, uint32_t fin);
// K13 (pow_pool_lift.hip), the table and the kernels of pow_pool_ancestors, pow_pool_fork_points and pow_pool_chain.
// up: the table's rows, cap words each, row j at up + (j - 1) cap; parent is its level 0.
hipError_t pow_launch_pool_lift_row(hipStream_t stream, const uint32_t* parent, uint32_t* up, uint32_t cap, uint32_t j,
                                    uint32_t first, uint32_t count, uint32_t size);
hipError_t pow_launch_pool_lift_small(hipStream_t stream, const uint32_t* parent, uint32_t* up, uint32_t cap,
                                      uint32_t rows, uint32_t first, uint32_t size);
hipError_t pow_launch_pool_lift_ancestor(hipStream_t stream, const PowLiftView& v, uint32_t k, const uint32_t* pos,
                                         const uint32_t* steps, uint32_t tip, uint32_t* out);
hipError_t pow_launch_pool_lift_fork(hipStream_t stream, const PowLiftView& v, uint32_t k, const uint32_t* a,
                                     const uint32_t* b, uint32_t* at, uint32_t* back_a, uint32_t* back_b);
// K14 (pow_pool_above.hip), the kernels of pow_pool_tips, pow_pool_subtrees and pow_pool_drop.  The marks lie in
// depth[1 - fin], as K12's.  _count is K12c and K12d behind each other on those marks.
hipError_t pow_launch_pool_above_child(hipStream_t stream, const PowPoolDev& D, uint32_t fin);
hipError_t pow_launch_pool_above_tip(hipStream_t stream, const PowPoolDev& D, uint32_t fin, uint32_t sound_only);
hipError_t pow_launch_pool_above_count(hipStream_t stream, const PowPoolDev& D, uint32_t fin);
hipError_t pow_launch_pool_above_gather(hipStream_t stream, const PowPoolDev& D, uint32_t fin);
hipError_t pow_launch_pool_above_subtree(hipStream_t stream, const PowPoolDev& D, uint32_t fin, const PowLiftView& v,
                                         const uint32_t* roots, uint32_t k, PowAboveAcc* acc, bool marks,
                                         uint32_t value);
// The launch sequences of K10, K12 and K13 that more than one caller queues (pow_api.cpp), each stated once: the
// library's calls and the test library's hooks run these.  As the wrappers above: a stream and views, the first
// failing hipError_t; none waits, records an event or copies to the host.
// `rounds` x K10d, then K10e on the buffers the last round wrote (rounds & 1).
hipError_t pow_queue_pool_rank(hipStream_t stream, const PowPoolDev& D, uint32_t rounds);
// The marks' reset (depth[fin ^ 1]), K12a, pow_pool_rounds(D.n) x K12b, K12c and K12d.
hipError_t pow_queue_pool_mark(hipStream_t stream, const PowPoolDev& D, uint32_t fin, const uint32_t* d_tips,
                               uint32_t n_tips, uint32_t min_index, uint32_t flags);
// The reset of T's control words and of its table, if it has one; then, if T keeps blocks, K12e, K12f and (with a
// table) K10b over T; otherwise, if want_map, F.next[0] filled with POW_POOL_NONE.
hipError_t pow_queue_pool_compact(hipStream_t stream, const PowPoolDev& F, const PowPoolDev& T, uint32_t cap,
                                  uint32_t fin, bool want_map);
// K13's table (`capacity` words a row) brought from the first `covered` blocks to `n`, from nothing if `stale`: K13b
// for at most POW_POOL_LIFT_SMALL new blocks, else K13a per old row over them; then every new row over all blocks.
// *launches is incremented per launch queued (pow_pool_lift_launches is its closed form), *work by its lanes.
hipError_t pow_queue_pool_lift(hipStream_t stream, const uint32_t* parent, uint32_t* up, uint32_t capacity,
                               uint32_t covered, uint32_t n, bool stale, uint32_t* launches, uint64_t* work);
// K14's two sequences.  The tips: the marks' reset, K14a, K14b, K12c, K12d and K14c; the list lies in next[0], its
// length in the control words' `marked`.
hipError_t pow_queue_pool_tips(hipStream_t stream, const PowPoolDev& D, uint32_t fin, uint32_t flags);
// The subtrees of k >= 1 roots (d_roots), behind a table that is up to date: the records' reset, and with `marks`
// the marks' (to 0; with `keep` then to 1 over the D.n blocks, the tail of the last word staying 0); K14d, whose
// members store 1, or 0 with `keep`; with `marks` K12c and K12d on what it left.
hipError_t pow_queue_pool_above(hipStream_t stream, const PowPoolDev& D, uint32_t fin, const PowLiftView& v,
                                const uint32_t* d_roots, uint32_t k, PowAboveAcc* d_acc, bool marks, bool keep);
hipError_t pow_sort_u32(void* temp, size_t* temp_bytes, uint32_t* keys, uint32_t* alt, uint32_t n,
                        uint32_t** sorted, hipStream_t stream);
hipError_t pow_launch_search_lat(bool full, bool any, bool asm_groups, unsigned grid, hipStream_t stream,
                                 const PowConstsLat& C, const PowLaunchLat& L, PowResult* res, PowResult* hout);

#pragma GCC visibility push(hidden)

// ... and pow_api.cpp's launches of K1' and K2' on the context's launch path.
int launch_search_lat(pow_ctx* ctx, bool full, bool any, bool asm_groups, unsigned grid, const PowLaunchLat& L,
                      uint64_t deadline_ns);
int launch_hash_one(pow_ctx* ctx, const PowMsg& M, uint32_t seq, uint64_t deadline_ns);

// The seam of the test library: null in libpow_gpu.so; libpow_gpu_test.so is
// the same objects plus pow_hooks.cpp, which points it at its table as the
// library loads.  Everything that reads a test or tuning switch from the
// environment, and the direct-dispatch launch path, is behind it.
struct pow_test_hooks {
  void (*configure)(pow_ctx* ctx);  // pow_init, before the allocations: the switches
  void (*open_path)(pow_ctx* ctx);  // pow_init, after them: the direct dispatcher, if asked for
  int (*before_launch)(pow_ctx* ctx);  // in front of a HIP launch (the stall kernel); POW_OK or an error
  // K1' / K2' by direct dispatch: 1 = sent, 0 = take the HIP path, < 0 = error (recorded)
  int (*dispatch_lat)(pow_ctx* ctx, bool full, bool any, bool asm_groups, unsigned grid, const PowLaunchLat& L,
                      uint64_t deadline_ns);
  int (*dispatch_hash_one)(pow_ctx* ctx, const PowMsg& M, uint32_t seq, uint64_t deadline_ns);
  // With ctx->aql set: the last packet (0 = completed, 1 = running, < 0 = minus
  // the queue's HSA status), and the watchdog's account of it.
  int (*path_status)(pow_ctx* ctx);
  std::string (*path_diag)(pow_ctx* ctx);
  int (*warm_path)(pow_ctx* ctx, const PowLaunchLat& L, const PowMsg& M);  // pow_warmup: the path's first packets
  bool (*close_path)(pow_ctx* ctx);  // pow_destroy; false = a packet may still write: free nothing
  // pow_group: a stand-in RCCL to load, if one is named (null + *why: it did not load)
  void* (*rccl_lib)(char* why, size_t cap);
};
extern const pow_test_hooks* pow_hooks;  // pow_api.cpp

#pragma GCC visibility pop
