// The test library's side of the seam (pow_ctx.h): linked into
// libpow_gpu_test.so only (build.py TEST_ONLY), never into the shipped
// libpow_gpu.so.  The test and tuning switches read from the environment at
// pow_init, the direct-dispatch launch path (pow_aql.cpp, POW_AQL=1), the stall
// kernel of the watchdog tests, the stand-in RCCL of the shard tests and
// the exports the shipped library does not have: pow_test_leading_zero_bits,
// pow_test_pool_rank, pow_test_pool_prune, pow_test_pool_lift and
// pow_test_pool_above (K10d/K10e, K12, K13 and K14 on trees of the caller's
// making, up to POW_POOL_MAX_BLOCKS nodes).  Those five stand on one frame
// (Frame: first error, buffers, copies, bounded waits); the three that take a
// forest share its check (check_forest) and, where they compact it, the
// prune's second half (compact_half).
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "pow_aql.h"
#include "pow_ctx.h"

hipError_t pow_launch_test_stall(hipStream_t stream, unsigned us, int realtime_khz);  // pow_test_kernels.hip
hipError_t pow_launch_test_lz(hipStream_t stream, const uint32_t* digests, uint32_t n, uint32_t* out);

namespace {

void configure(pow_ctx* ctx) {
  if (const char* ff = getenv("POW_FORCE_FULL")) ctx->force_full = ff[0] == '1';
  if (const char* fi = getenv("POW_FAULT_INJECT"))
    ctx->fault_mine = std::strcmp(fi, "mine") == 0 ? "injected fault (POW_FAULT_INJECT=mine)" : nullptr;
  if (const char* lm = getenv("POW_LAT_MAX")) ctx->lat_max = std::min<uint64_t>(strtoull(lm, nullptr, 0), 1ull << 31);
  if (const char* lw = getenv("POW_LAT_WPS")) ctx->lat_wps = (unsigned)std::min(8ul, strtoul(lw, nullptr, 0));
  if (const char* si = getenv("POW_TEST_SENTINEL_IDLE")) ctx->sentinel_idle = si[0] == '1';
  if (const char* ts = getenv("POW_TEST_STALL_US")) ctx->test_stall_us = (unsigned)strtoul(ts, nullptr, 0);
  // pow_mine_chain: blocks per batch, and the highest d on the fused path (-1: the host loop at every d)
  if (const char* cb = getenv("POW_CHAIN_BATCH")) ctx->chain_batch = (unsigned)std::min(64ul, strtoul(cb, nullptr, 0));
  if (const char* cf = getenv("POW_CHAIN_FUSED_MAX")) ctx->chain_fused_max = (int)std::max(-1l, std::min(32l, strtol(cf, nullptr, 0)));
  // K4's grid: lanes = 2^n times the expected trials (the result must not depend on it)
  if (const char* cl = getenv("POW_CHAIN_LANES_LOG2")) ctx->chain_lanes_log2 = (unsigned)std::min(8ul, strtoul(cl, nullptr, 0));
  // pow_mine_batch: the highest d on the fused path (-1: the host loop at every d), templates per
  // launch (the workgroup and window caps still hold) and K5's lanes per template (as K4's; unset: the plan)
  if (const char* bf = getenv("POW_BATCH_FUSED_MAX")) ctx->batch_fused_max = (int)std::max(-1l, std::min(32l, strtol(bf, nullptr, 0)));
  if (const char* bt = getenv("POW_BATCH_TILE")) ctx->batch_tile = (unsigned)std::min((unsigned long)POW_BATCH_MAX_TILE, strtoul(bt, nullptr, 0));
  if (const char* bl = getenv("POW_BATCH_LANES_LOG2")) ctx->batch_lanes_log2 = (int)std::min(8ul, strtoul(bl, nullptr, 0));
  // pow_mine_race: the highest d on the fused path (-1: the host loop at every d), heights per batch
  // (the window cap still holds) and K6's lanes over all rivals (as K4's)
  if (const char* rf = getenv("POW_RACE_FUSED_MAX")) ctx->race_fused_max = (int)std::max(-1l, std::min(32l, strtol(rf, nullptr, 0)));
  if (const char* rb = getenv("POW_RACE_BATCH")) ctx->race_batch = (unsigned)std::min((unsigned long)POW_RACE_MAX_BATCH, strtoul(rb, nullptr, 0));
  if (const char* rl = getenv("POW_RACE_LANES_LOG2")) ctx->race_lanes_log2 = (unsigned)std::min(8ul, strtoul(rl, nullptr, 0));
  // pow_mine_rand: K8's run T (rounded down to a power of two, at most 1,024), its grid (2^n lanes, at
  // least one workgroup and at most one per CU) and the trials per launch (2^n, at most 2^26); the
  // result must not depend on any of them
  if (const char* rr = getenv("POW_RAND_RUN")) ctx->rand_run = (unsigned)std::min((unsigned long)POW_RAND_MAX_RUN, strtoul(rr, nullptr, 0));
  if (const char* rg = getenv("POW_RAND_LANES_LOG2")) ctx->rand_lanes_log2 = (int)std::min(16ul, strtoul(rg, nullptr, 0));
  if (const char* rn = getenv("POW_RAND_LAUNCH_LOG2")) ctx->rand_launch_log2 = (unsigned)std::min(26ul, strtoul(rn, nullptr, 0));
  // pow_find_seed: K9's run T (rounded down to 31 x 2^j, 31 to 992), its workgroups per seed (1 to 256)
  // and the (seed, trial) pairs per launch (2^n, at most 2^30); the result must not depend on any of them
  if (const char* sr = getenv("POW_SEED_RUN")) ctx->seed_run = (unsigned)std::min(992ul, strtoul(sr, nullptr, 0));
  if (const char* sw = getenv("POW_SEED_WG")) ctx->seed_wg = (unsigned)std::min((unsigned long)POW_RAND_MAX_WG, strtoul(sw, nullptr, 0));
  if (const char* sn = getenv("POW_SEED_LAUNCH_LOG2")) ctx->seed_launch_log2 = (unsigned)std::min((unsigned long)POW_SEED_LAUNCH_LOG2, strtoul(sn, nullptr, 0));
  // pow_index_blocks: the table's slots (2^n, never below the pool's blocks + 1); the result must not depend on it
  if (const char* ps = getenv("POW_POOL_SLOTS_LOG2")) ctx->pool_slots_log2 = (unsigned)std::min(21ul, strtoul(ps, nullptr, 0));
  // pow_pool_open: that switch also gives a pool's first table (2^n slots; every add keeps at least two slots per
  // block), and this one its first capacity in blocks when reserve is 0; the results must not depend on either
  if (const char* pc = getenv("POW_POOL_FIRST_CAP")) ctx->pool_first_cap = (unsigned)std::min((unsigned long)POW_POOL_MAX_BLOCKS, strtoul(pc, nullptr, 0));
  if (const char* g = getenv("POW_GRID_PER_CU")) {  // launch-geometry experiments
    const int per = atoi(g);
    if (per > 0 && per <= 64) ctx->grid_full = (unsigned)ctx->cu_count * (unsigned)per;
  }
  // POW_WATCHDOG_MS: the watchdog's base deadline (tests of the watchdog itself)
  if (const char* wd = getenv("POW_WATCHDOG_MS")) ctx->watchdog_ns = std::max(1ull, strtoull(wd, nullptr, 0)) * 1000000ull;
}

// POW_AQL=1: K1'/K2' as AQL packets (pow_aql.cpp; dispatch A/B and the
// multi-producer ordering test), POW_AQL_EXP its experiment flags.
void open_path(pow_ctx* ctx) {
  const char* use_aql = getenv("POW_AQL");
  const unsigned aql_flags = getenv("POW_AQL_EXP") ? (unsigned)strtoul(getenv("POW_AQL_EXP"), nullptr, 0) : 0u;
  if (use_aql && use_aql[0] == '1' && pow_aql_open(ctx->device, aql_flags, &ctx->aql, &ctx->aql_why) != 0)
    ctx->aql = nullptr;  // the HIP launch path
}

int before_launch(pow_ctx* ctx) {
  if (ctx->test_stall_us) HIP_OK(pow_launch_test_stall(ctx->stream, ctx->test_stall_us, ctx->realtime_khz));
  return POW_OK;
}

// The explicit kernel arguments of a direct dispatch (pow_aql.cpp): the
// parameters in declaration order, each at its natural alignment.
struct ArgPack {
  alignas(8) uint8_t b[2048];
  uint32_t n = 0;
  template <class T>
  void put(const T& v) {
    n = (n + (uint32_t)alignof(T) - 1) & ~((uint32_t)alignof(T) - 1);
    memcpy(b + n, &v, sizeof v);
    n += (uint32_t)sizeof v;
  }
};

// A context whose direct-dispatch queue has reported an error goes back to
// the HIP launch path for good (pow_launch_path then says so).
bool aql_usable(pow_ctx* ctx) {
  if (!ctx->aql) return false;
  if (pow_aql_status(ctx->aql) >= 0) return true;
  ctx->aql_why = "the dispatch queue reported an error; back on the HIP launch path";
  if (!pow_aql_close(ctx->aql)) ctx->wedged = ctx->aql_lost = true;  // a packet may still be in flight
  ctx->aql = nullptr;
  return false;
}

// One packet through the context's dispatcher: 1 = sent.  A refused packet may
// have left its reserved slot behind (pow_aql_dispatch): the context is wedged.
int send_packet(pow_ctx* ctx, int kernel, const char* name, uint32_t grid, uint32_t wg, const ArgPack& a,
                uint64_t deadline_ns) {
  std::string why;
  if (!pow_aql_dispatch(ctx->aql, kernel, grid, wg, a.b, a.n, deadline_ns, &why)) return 1;
  ctx->wedged = true;
  return fail(POW_EHIP, "dispatch of %s failed: %s (%s)", name, why.c_str(), pow_aql_diag(ctx->aql).c_str());
}

int dispatch_lat(pow_ctx* ctx, bool full, bool any, bool asm_groups, unsigned grid, const PowLaunchLat& L,
                 uint64_t deadline_ns) {
  if (!aql_usable(ctx)) return 0;
  ArgPack a;
  a.put(ctx->lat_consts);
  a.put(L);
  a.put(ctx->d_lat);
  a.put(ctx->d_lat_host);
  const int k = POW_AQL_LAT0 + (full ? 1 : 0) + (any ? 2 : 0) + (asm_groups ? 4 : 0);
  return send_packet(ctx, k, "pow_search_lat", grid, 256, a, deadline_ns);
}

int dispatch_hash_one(pow_ctx* ctx, const PowMsg& M, uint32_t seq, uint64_t deadline_ns) {
  if (!aql_usable(ctx)) return 0;
  ArgPack a;
  a.put(M);
  a.put(ctx->d_one);
  a.put(seq);
  return send_packet(ctx, POW_AQL_HASH_ONE, "pow_hash_one", 1, 64, a, deadline_ns);
}

int path_status(pow_ctx* ctx) { return pow_aql_status(ctx->aql); }

std::string path_diag(pow_ctx* ctx) { return "launch path direct, " + pow_aql_diag(ctx->aql); }

// The warm-up launches once more through the direct-dispatch queue (its first packets).
int warm_path(pow_ctx* ctx, const PowLaunchLat& L, const PowMsg& M) {
  if (!ctx->aql) return POW_OK;
  for (int k = 0; k < 9; ++k) {
    const uint64_t deadline = mono_ns() + ctx->watchdog_ns;
    if (int rc = k < 8 ? launch_search_lat(ctx, k & 1, k & 2, k & 4, 1, L, deadline)
                       : launch_hash_one(ctx, M, 0, deadline))
      return rc;
    for (int st, n = 0; (st = pow_aql_status(ctx->aql)) != 0; ++n) {
      if (st < 0) return fail(POW_EHIP, "warm-up dispatch: queue error 0x%x", -st);
      if (n > 20000) break;  // POW_AQL_EXP_NO_SIGNAL: no completion to wait for; ~20 ms
      std::this_thread::sleep_for(std::chrono::microseconds(1));
    }
  }
  return POW_OK;
}

// Direct-dispatch packets, which the stream does not see, are waited for on
// the dispatcher's completion signal (pow_aql_close).
bool close_path(pow_ctx* ctx) { return !ctx->aql_lost && pow_aql_close(ctx->aql); }

// A stand-in RCCL (tests/stub_rccl) that reduces over POSIX shared memory, so
// pow_group_init's RCCL leg runs with several ranks on the one GPU of a test
// box (RCCL refuses two ranks per GPU).
void* rccl_lib(char* why, size_t cap) {
  const char* p = getenv("POW_TEST_RCCL_LIB");
  if (!p) return nullptr;
  void* h = dlopen(p, RTLD_NOW | RTLD_LOCAL);
  if (!h) snprintf(why, cap, "cannot load POW_TEST_RCCL_LIB %s: %s", p, dlerror());
  return h;
}

const pow_test_hooks kHooks = {configure,   open_path, before_launch, dispatch_lat, dispatch_hash_one,
                               path_status, path_diag, warm_path,     close_path,   rccl_lib};
const bool kRegistered = (pow_hooks = &kHooks, true);  // as the library loads

// The frame of the exports below: the first error of a hook's HIP calls (rc),
// the device buffers it made, its copies and its bounded waits.  Nothing is
// reported behind the first error, and `up` and `down` queue nothing behind it,
// nor for a null host pointer or no bytes.  The buffers are freed as the frame
// goes, unless a wait failed and left the context wedged: after a watchdog the
// launches may still write.
struct Frame {
  pow_ctx* const ctx;
  int rc = POW_OK;
  bool wait_failed = false;
  std::vector<void*> owned;
  explicit Frame(pow_ctx* c) : ctx(c) {}
  Frame(const Frame&) = delete;
  ~Frame() {
    if (wait_failed && ctx->wedged) return;
    for (void* d : owned) (void)hipFree(d);
  }
  void step(hipError_t e, const char* what) {
    if (rc == POW_OK && e != hipSuccess) rc = fail(POW_EHIP, "%s failed: %s", what, hipGetErrorString(e));
  }
  uint32_t* alloc(size_t words) {
    void* d = nullptr;
    step(hipMalloc(&d, words * sizeof(uint32_t)), "hipMalloc");
    if (d) owned.push_back(d);
    return (uint32_t*)d;
  }
  void up(void* dst, const void* src, size_t bytes) {
    if (rc == POW_OK && src && bytes) step(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream), "copy in");
  }
  void down(void* dst, const void* src, size_t bytes) {
    if (rc == POW_OK && dst && bytes) step(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream), "copy out");
  }
  // Every hook waits even after a failed step: the copies queued so far read and write host memory.
  int wait(const char* what, uint64_t extra_ns) {
    const int waited = pow_ctx_stream_wait(ctx, what, extra_ns);
    wait_failed = wait_failed || waited != POW_OK;
    if (rc == POW_OK) rc = waited;
    return rc;
  }
};

// The forest of pow_test_pool_prune, _lift and _above, behind the size and the
// hook's own scalars (which its refusals name first): `arrays` says that none
// of the hook's input arrays is null; every parent is a node or an end.
int check_forest(size_t n, bool arrays, const uint32_t* parent) {
  if (!arrays && n) return fail(POW_EINVAL, "null");
  for (size_t i = 0; i < n; ++i)
    if (parent[i] >= n && parent[i] < POW_POOL_NONE)
      return fail(POW_EINVAL, "parent %u of node %zu is neither a node nor an end", parent[i], i);
  return POW_OK;
}

// The second half of pow_test_pool_prune and of pow_test_pool_above's mode 2, as
// pool_compact (pow_api.cpp) runs it on a pool: `kept` < F.n marks stand in
// F as the first half left them; new arrays at pow_pool_prune_cap's capacity
// and pow_queue_pool_compact over a view with no table (K12e, K12f; K10b is
// not run; nothing marked: the map is POW_POOL_NONE throughout, as the
// library's reset makes it), the map and the survivors' parent and depth
// down, what `more` queues of the survivors' view, and the second bounded wait.
template <class More>
int compact_half(Frame& f, const char* what, const PowPoolDev& F, uint32_t kept, uint32_t fin, uint32_t* map,
                 uint32_t* parent_out, uint32_t* depth_out, More more) {
  pow_ctx* const ctx = f.ctx;
  const uint32_t cap = pow_pool_prune_cap(kept, pow_pool_live_first_cap(0, ctx->pool_first_cap));
  const PowPoolLivePlan to = pow_pool_live_plan(cap);
  uint32_t* const to_base = f.alloc(to.words);
  if (f.rc != POW_OK) return f.rc;
  const PowPoolDev T = pow_pool_live_dev(to_base, to, nullptr, kept, 0);
  const size_t kw = (size_t)kept * sizeof(uint32_t);
  f.step(pow_queue_pool_compact(ctx->stream, F, T, cap, fin, map != nullptr), "K12e, K12f");  // no table: no K10b
  f.down(map, F.next[0], (size_t)F.n * sizeof(uint32_t)), f.down(parent_out, T.parent, kw), f.down(depth_out, T.depth[fin], kw);
  more(T);
  return f.wait(what, 100ull * (F.n + 2ull * kept));
}

}  // namespace

// The kernels' leading-zero count (sha256_dev.h leading_zero_bits) of n digests
// of the caller's choosing: digests = n x 8 words, most significant first;
// out = n counts.  One launch of pow_test_lz on the context's stream.
extern "C" int pow_test_leading_zero_bits(pow_ctx* ctx, const uint32_t* digests, size_t n, uint32_t* out) {
  if (!ctx || ((!digests || !out) && n)) return fail(POW_EINVAL, "null");
  if (n > (1u << 20)) return fail(POW_EINVAL, "too many digests (%zu > 2^20)", n);
  if (n == 0) return POW_OK;
  HIP_OK(hipSetDevice(ctx->device));
  Frame f(ctx);
  uint32_t* const d_in = f.alloc(n * 8);
  uint32_t* const d_out = f.alloc(n);
  f.up(d_in, digests, n * 32);
  if (f.rc == POW_OK) f.step(pow_launch_test_lz(ctx->stream, d_in, (uint32_t)n, d_out), "pow_test_lz");
  f.down(out, d_out, n * 4);
  return f.rc == POW_OK ? f.wait("pow_test_lz", 0) : f.rc;  // nothing is queued behind a failed step
}

// K10d and K10e (pow_pool.hip) on a next[] of the caller's choosing, the only
// way to rank a cycle: next[i] is a position below n or anything at or above n
// (the end of a walk), every node counts 1 and none is flagged.  depth_out and
// n_bad_out = n words each: what pow_index_blocks would give for that tree.
extern "C" int pow_test_pool_rank(pow_ctx* ctx, const uint32_t* next, size_t n, uint32_t* depth_out, uint32_t* n_bad_out) {
  if (!ctx || ((!next || !depth_out || !n_bad_out) && n)) return fail(POW_EINVAL, "null");
  if (n > POW_POOL_MAX_BLOCKS) return fail(POW_EINVAL, "too many nodes (%zu > 2^20)", n);
  if (n == 0) return POW_OK;
  HIP_OK(hipSetDevice(ctx->device));
  const PowPoolPlan plan = pow_pool_plan((uint32_t)n, 0);
  const size_t words = n * sizeof(uint32_t);
  Frame f(ctx);
  uint32_t* const base = f.alloc(plan.words);
  if (f.rc != POW_OK) return f.rc;
  const PowPoolDev D = pow_pool_dev(base, plan, (uint32_t)n);
  const uint32_t last = plan.rounds & 1u;
  std::vector<uint32_t> ones(n, 1u);
  f.step(hipMemsetAsync(base, 0, plan.words * sizeof(uint32_t), ctx->stream), "reset");  // status, index, bad, ctl: all zero
  f.up(D.next[0], next, words), f.up(D.depth[0], ones.data(), words);
  if (f.rc == POW_OK) f.step(pow_queue_pool_rank(ctx->stream, D, plan.rounds), "K10d, K10e");
  f.down(depth_out, D.depth[last], words), f.down(n_bad_out, D.bad[last], words);
  // waited for even after a failed step: the copies queued so far read `ones`
  return f.wait("pow_test_pool_rank", 100ull * n * (plan.rounds + 1u));
}

// What pow_test_pool_prune takes and gives: arrays of n entries unless said.
// An output that is null is not written.
struct pow_test_prune_io {
  // in: a forest of the caller's making, as K10 and K11 would have left it
  const uint32_t* parent;  // a position below n, POW_POOL_ROOT or POW_POOL_NONE
  const uint32_t* index;
  const uint32_t* n_bad;
  const uint8_t* status;
  const uint32_t* depth;
  const uint32_t* digest;  // 8 n words; null: zeros
  const uint32_t* prev;    // 8 n words; null: zeros
  const uint32_t* tips;    // n_tips positions below n
  size_t n_tips;
  uint32_t min_index, flags;  // POW_KEEP_BY_INDEX, POW_KEEP_SOUND_ONLY
  uint32_t fin;            // 0 or 1: which of depth[], bad[] hold the final values; the others are the scratch
  // out
  uint8_t* marks;          // K12a and K12b
  uint32_t* kept;          // one word: K12d's total
  uint32_t* map;           // K12e's newpos, or K12a's own positions when nothing is dropped
  // the first `kept` entries of each (room for n): what K12e and K12f left, or the input when nothing is dropped
  uint32_t* parent_out;
  uint32_t* index_out;
  uint32_t* depth_out;
  uint32_t* n_bad_out;
  uint8_t* status_out;
  uint32_t* digest_out;    // 8 words a block
  uint32_t* prev_out;      // 8 words a block
  unsigned long long* best;  // one word: the new control words' key (K12f), 0 when nothing is dropped
  uint32_t* n_flagged;     // one word: K12f's count, 0 when nothing is dropped
};
static_assert(sizeof(pow_test_prune_io) == 23 * 8, "tests/pool_deep_util.py PruneIO");

// K12 (pow_pool_prune.hip) on a forest of the caller's choosing, with no pool
// and no table: the mark's launches (pow_queue_pool_mark, as pool_mark_run
// queues them) in one section, then by K12d's total, as pow_pool_prune decides
// it: everything marked, and K12a's positions are the map; otherwise
// compact_half.  Two bounded waits, one per section: the second section's grid
// is the first's result.  The scratch is pool_mark_run's: marks in
// depth[1 - fin], positions in bad[1 - fin], the walks in next[], the partials
// in next[1].
extern "C" int pow_test_pool_prune(pow_ctx* ctx, size_t n, const pow_test_prune_io* io) {
  if (n > POW_POOL_MAX_BLOCKS) return fail(POW_EINVAL, "too many nodes (%zu > 2^20)", n);
  if (!ctx || !io) return fail(POW_EINVAL, "null");
  if (io->flags & ~(uint32_t)(POW_KEEP_BY_INDEX | POW_KEEP_SOUND_ONLY)) return fail(POW_EINVAL, "unknown flags 0x%x", io->flags);
  if (io->fin > 1u) return fail(POW_EINVAL, "fin %u > 1", io->fin);
  if (io->n_tips > POW_POOL_MAX_TIPS) return fail(POW_EINVAL, "too many tips (%zu > %u)", io->n_tips, POW_POOL_MAX_TIPS);
  if (!io->tips && io->n_tips) return fail(POW_EINVAL, "null tips");
  for (size_t k = 0; k < io->n_tips; ++k)
    if (io->tips[k] >= n) return fail(POW_EINVAL, "tip %zu (node %u) past the forest's %zu", k, io->tips[k], n);
  if (int rc = check_forest(n, io->parent && io->index && io->n_bad && io->status && io->depth, io->parent)) return rc;
  if (n == 0) return POW_OK;
  HIP_OK(hipSetDevice(ctx->device));
  const uint32_t n32 = (uint32_t)n, n_tips = (uint32_t)io->n_tips, fin = io->fin, rounds = pow_pool_rounds(n32);
  const PowPoolLivePlan from = pow_pool_live_plan(n32);
  const size_t words = (size_t)n32 * sizeof(uint32_t);
  PowPoolLiveCtl ctl{}, new_ctl{};
  Frame f(ctx);
  uint32_t* const base = f.alloc(from.words);
  uint32_t* const d_tips = f.alloc(std::max<size_t>(n_tips, 1));
  if (f.rc != POW_OK) return f.rc;
  const PowPoolDev F = pow_pool_live_dev(base, from, nullptr, n32, 0);
  f.step(hipMemsetAsync(base, 0, from.words * sizeof(uint32_t), ctx->stream), "reset");  // kind, and a null digest or prev
  f.up(F.parent, io->parent, words), f.up(F.index, io->index, words), f.up(F.bad[fin], io->n_bad, words);
  f.up(F.depth[fin], io->depth, words), f.up(F.status, io->status, n), f.up(F.dig, io->digest, 8 * words);
  f.up(F.prev, io->prev, 8 * words), f.up(d_tips, io->tips, n_tips * sizeof(uint32_t));
  if (f.rc == POW_OK) {  // pool_mark_run's section
    f.step(pow_queue_pool_mark(ctx->stream, F, fin, d_tips, n_tips, io->min_index, io->flags), "K12a to K12d");
    f.down(&ctl, F.ctl, sizeof ctl), f.down(io->marks, F.depth[fin ^ 1u], n);
  }
  if (f.wait("pow_test_pool_prune (mark)", 100ull * n * (rounds + 3ull)) != POW_OK) return f.rc;
  const uint32_t kept = ctl.marked;
  if (kept > n32) return fail(POW_EHIP, "K12d counted %u marks on %u nodes", kept, n32);
  if (io->kept) *io->kept = kept;
  if (io->best) *io->best = 0;
  if (io->n_flagged) *io->n_flagged = 0;
  if (kept == n32) {  // nothing to drop: the arrays stay as they are
    f.down(io->map, F.bad[fin ^ 1u], words), f.down(io->parent_out, F.parent, words), f.down(io->index_out, F.index, words);
    f.down(io->depth_out, F.depth[fin], words), f.down(io->n_bad_out, F.bad[fin], words), f.down(io->status_out, F.status, n);
    f.down(io->digest_out, F.dig, 8 * words), f.down(io->prev_out, F.prev, 8 * words);
    return f.wait("pow_test_pool_prune (map)", 100ull * n);
  }
  const int rc = compact_half(f, "pow_test_pool_prune (gather)", F, kept, fin, io->map, io->parent_out, io->depth_out,
                              [&](const PowPoolDev& T) {
                                const size_t kw = (size_t)kept * sizeof(uint32_t);
                                f.down(&new_ctl, T.ctl, sizeof new_ctl), f.down(io->index_out, T.index, kw);
                                f.down(io->n_bad_out, T.bad[fin], kw), f.down(io->status_out, T.status, kept);
                                f.down(io->digest_out, T.dig, 8 * kw), f.down(io->prev_out, T.prev, 8 * kw);
                              });
  if (rc == POW_OK) {
    if (io->best) *io->best = new_ctl.k10.best;
    if (io->n_flagged) *io->n_flagged = new_ctl.k10.n_flagged;
  }
  return rc;
}

// What pow_test_pool_lift takes and gives.
struct pow_test_lift_io {
  const uint32_t* parent;  // n: a position below n, POW_POOL_ROOT or POW_POOL_NONE; the first `covered` closed under it
  const uint32_t* depth;   // n: the nodes on the walk from each, itself included
  uint32_t covered;        // the table covered this many nodes before the call (0: it is made from nothing)
  uint32_t capacity;       // words of a row, n..POW_POOL_MAX_BLOCKS
  uint32_t mode;           // 0: k ancestor queries (in0 = pos, in1 = steps); 1: k pairs (in0 = a, in1 = b);
                           // 2: the chain of `tip`, k <= n answers
  const uint32_t* in0;
  const uint32_t* in1;
  uint32_t tip;
  size_t k;                // 0: the table alone, no query launch
  uint32_t* out0;          // k answers (mode 1: at); mode 2: k answers and the length word behind them
  uint32_t* out1;          // mode 1: back_a
  uint32_t* out2;          // mode 1: back_b
  uint32_t* launches;      // one word: the table's launches of the query call (the table at `covered` is not counted)
  uint32_t* table;         // null, or pow_pool_lift_rows(n) x n words: row j at (j - 1) n
};
static_assert(sizeof(pow_test_lift_io) == 13 * 8, "tests/pool_deep_util.py LiftIO");

// K13 (pow_pool_lift.hip) on a parent and a depth array of the caller's making,
// with no pool: the table as a pool of `covered` nodes had it, then the query
// calls' update to a pool of n nodes (both pow_queue_pool_lift, the statement
// pool_lift_update runs), then one query launch, K13c or K13d.  The
// table is allocated at `capacity` words a row, as the pool's, and filled with
// 0xEE bytes first: an entry no launch wrote shows in `table`, and as a value it
// is past every size, so no walk takes it for a position.
extern "C" int pow_test_pool_lift(pow_ctx* ctx, size_t n, const pow_test_lift_io* io) {
  if (n > POW_POOL_MAX_BLOCKS) return fail(POW_EINVAL, "too many nodes (%zu > 2^20)", n);
  if (!ctx || !io) return fail(POW_EINVAL, "null");
  if (io->capacity < n || io->capacity > POW_POOL_MAX_BLOCKS)
    return fail(POW_EINVAL, "capacity %u outside %zu..2^20", io->capacity, n);
  if (io->covered > n) return fail(POW_EINVAL, "covered %u past the forest's %zu", io->covered, n);
  if (io->mode > 2u) return fail(POW_EINVAL, "unknown mode %u", io->mode);
  if (io->k > (io->mode == 2u ? n : (size_t)POW_POOL_MAX_BLOCKS))
    return fail(POW_EINVAL, "too many queries (%zu > %zu)", io->k, io->mode == 2u ? n : (size_t)POW_POOL_MAX_BLOCKS);
  if (io->k && (!io->out0 || (io->mode != 2u && (!io->in0 || !io->in1)) || (io->mode == 1u && (!io->out1 || !io->out2))))
    return fail(POW_EINVAL, "null");
  for (size_t q = 0; q < io->k && io->mode != 2u; ++q)
    if (io->in0[q] >= n || (io->mode == 1u && io->in1[q] >= n))
      return fail(POW_EINVAL, "query %zu names a node past the forest's %zu", q, n);
  if (io->mode == 2u && io->k && io->tip >= n) return fail(POW_EINVAL, "tip (node %u) past the forest's %zu", io->tip, n);
  if (int rc = check_forest(n, io->parent && io->depth, io->parent)) return rc;
  for (size_t i = 0; i < io->covered; ++i)
    if (io->parent[i] >= io->covered && io->parent[i] < n)
      return fail(POW_EINVAL, "the first %u nodes are not closed under parent (node %zu, parent %u)", io->covered, i,
                  io->parent[i]);
  if (io->launches) *io->launches = 0;
  if (n == 0) return POW_OK;
  HIP_OK(hipSetDevice(ctx->device));
  const uint32_t n32 = (uint32_t)n, cap = io->capacity, covered = io->covered, k = (uint32_t)io->k;
  const uint32_t rows = pow_pool_lift_rows(n32);
  const size_t words = (size_t)n32 * sizeof(uint32_t), kb = (size_t)k * sizeof(uint32_t);
  const size_t up_words = std::max<size_t>((size_t)cap * pow_pool_lift_rows(cap), 1);
  Frame f(ctx);
  uint32_t* const d_parent = f.alloc(n32);
  uint32_t* const d_depth = f.alloc(n32);
  uint32_t* const d_up = f.alloc(up_words);
  uint32_t* const d_io = f.alloc(5 * (size_t)k + 1);  // in0, in1, then the results, as pool_lift_run lays them out
  uint32_t launches = 0;
  uint64_t work = 0;
  if (f.rc == POW_OK) {
    f.step(hipMemsetAsync(d_up, 0xEE, up_words * sizeof(uint32_t), ctx->stream), "reset");
    f.up(d_parent, io->parent, words), f.up(d_depth, io->depth, words);
    // the table a pool of `covered` nodes had: made from nothing at that size; its launches are not reported
    uint32_t before = 0;
    if (f.rc == POW_OK && covered)
      f.step(pow_queue_pool_lift(ctx->stream, d_parent, d_up, cap, 0, covered, true, &before, &work), "K13a");
    // the query call's update, stale when nothing was covered
    if (f.rc == POW_OK)
      f.step(pow_queue_pool_lift(ctx->stream, d_parent, d_up, cap, covered, n32, covered == 0, &launches, &work), "K13a, K13b");
  }
  if (f.rc == POW_OK && k) {
    uint32_t* const d_in0 = d_io;
    uint32_t* const d_in1 = d_io + k;
    uint32_t* const d_out = d_in1 + k;
    const PowLiftView v{d_parent, d_depth, d_up, cap, n32, pow_pool_rounds(n32)};
    if (io->mode != 2u) f.up(d_in0, io->in0, kb), f.up(d_in1, io->in1, kb);
    if (io->mode == 1u) {
      f.step(pow_launch_pool_lift_fork(ctx->stream, v, k, d_in0, d_in1, d_out, d_out + k, d_out + 2 * (size_t)k), "K13d");
      f.down(io->out0, d_out, kb), f.down(io->out1, d_out + k, kb), f.down(io->out2, d_out + 2 * (size_t)k, kb);
    } else {
      const bool chain = io->mode == 2u;
      f.step(pow_launch_pool_lift_ancestor(ctx->stream, v, k, chain ? nullptr : d_in0, d_in1, io->tip, d_out), "K13c");
      f.down(io->out0, d_out, kb + (chain ? sizeof(uint32_t) : 0));
    }
  }
  for (uint32_t j = 1; io->table && j <= rows; ++j)
    f.down(io->table + (size_t)(j - 1u) * n32, d_up + (size_t)(j - 1u) * cap, words);
  // + 100 ns per node and launch
  const int rc = f.wait("pow_test_pool_lift", 100ull * (work + k + (io->table ? (uint64_t)n32 * rows : 0)));
  if (rc == POW_OK && io->launches) *io->launches = launches;
  return rc;
}

// What pow_test_pool_above takes and gives: arrays of n entries unless said.
// An output that is null is not written.
struct pow_test_above_io {
  // in: a forest of the caller's making, as K10 and K11 would have left it (every status 0)
  const uint32_t* parent;  // a position below n, POW_POOL_ROOT or POW_POOL_NONE
  const uint32_t* depth;   // the nodes on the walk from each, itself included
  const uint32_t* index;
  const uint32_t* n_bad;
  const uint32_t* roots;   // k positions below n (modes 1 and 2)
  size_t k;                // 1..POW_POOL_MAX_ROOTS in modes 1 and 2
  uint32_t mode;           // 0: pow_pool_tips; 1: pow_pool_subtrees with on[]; 2: pow_pool_drop
  uint32_t flags;          // mode 0: POW_TIPS_SOUND_ONLY
  uint32_t fin;            // 0 or 1: which of depth[], bad[] hold the final values; the others are the scratch
  uint32_t pad;
  // out
  uint8_t* marks;          // mode 0: the tip marks; 1: on[]; 2: the keep-marks
  uint32_t* total;         // one word: K12d's total of those marks
  uint32_t* list;          // mode 0: K14c's list, the first `total` entries (room for n)
  uint32_t* size;          // modes 1, 2: k each, K14d's records
  uint32_t* height;
  unsigned long long* best;  // k: the key as K14d left it (0: none)
  uint32_t* map;           // mode 2: K12e's newpos
  uint32_t* parent_out;    // mode 2: the first `total` entries of what K12e and K12f left
  uint32_t* depth_out;
};
static_assert(sizeof(pow_test_above_io) == 17 * 8, "tests/pool_above_util.py AboveIO");

// K14 (pow_pool_above.hip) on a forest of the caller's choosing, with no pool,
// no hashing and no name table: the library's own sequences.  Mode 0:
// pow_queue_pool_tips.  Modes 1 and 2: K13's table made from nothing
// (pow_queue_pool_lift), then pow_queue_pool_above, as pool_above_run queues
// them; mode 2 goes on as pow_pool_drop does, by K12d's total (a root is
// dropped with its subtree, so never everything kept), through compact_half.
extern "C" int pow_test_pool_above(pow_ctx* ctx, size_t n, const pow_test_above_io* io) {
  if (n > POW_POOL_MAX_BLOCKS) return fail(POW_EINVAL, "too many nodes (%zu > 2^20)", n);
  if (!ctx || !io) return fail(POW_EINVAL, "null");
  if (io->mode > 2u) return fail(POW_EINVAL, "unknown mode %u", io->mode);
  if (io->flags & ~(uint32_t)POW_TIPS_SOUND_ONLY) return fail(POW_EINVAL, "unknown flags 0x%x", io->flags);
  if (io->fin > 1u) return fail(POW_EINVAL, "fin %u > 1", io->fin);
  if (io->mode && (io->k == 0 || io->k > POW_POOL_MAX_ROOTS || !io->roots))
    return fail(POW_EINVAL, "1..%d roots", POW_POOL_MAX_ROOTS);
  for (size_t q = 0; io->mode && q < io->k; ++q)
    if (io->roots[q] >= n) return fail(POW_EINVAL, "root %zu (node %u) past the forest's %zu", q, io->roots[q], n);
  if (int rc = check_forest(n, io->parent && io->depth && io->index && io->n_bad, io->parent)) return rc;
  if (n == 0) return POW_OK;
  HIP_OK(hipSetDevice(ctx->device));
  const uint32_t n32 = (uint32_t)n, fin = io->fin, k = io->mode ? (uint32_t)io->k : 0u;
  const PowPoolLivePlan from = pow_pool_live_plan(n32);
  const size_t words = (size_t)n32 * sizeof(uint32_t);
  const size_t up_words = std::max<size_t>((size_t)n32 * pow_pool_lift_rows(n32), 1);
  std::vector<PowAboveAcc> acc(std::max<uint32_t>(k, 1));
  PowPoolLiveCtl ctl{};
  Frame f(ctx);
  uint32_t* const base = f.alloc(from.words);
  uint32_t* const d_up = f.alloc(up_words);
  uint32_t* const d_find = f.alloc(5 * (size_t)std::max<uint32_t>(k, 1));  // the k records, then the roots, as pool_above_run lays them out
  if (f.rc != POW_OK) return f.rc;
  const PowPoolDev F = pow_pool_live_dev(base, from, nullptr, n32, 0);
  PowAboveAcc* const d_acc = (PowAboveAcc*)d_find;
  uint32_t* const d_roots = d_find + 4 * (size_t)k;
  f.step(hipMemsetAsync(base, 0, from.words * sizeof(uint32_t), ctx->stream), "reset");  // status, kind, digests, names
  f.step(hipMemsetAsync(d_up, 0xEE, up_words * sizeof(uint32_t), ctx->stream), "reset");  // past every size, as the lift hook's
  f.up(F.parent, io->parent, words), f.up(F.index, io->index, words), f.up(F.bad[fin], io->n_bad, words);
  f.up(F.depth[fin], io->depth, words), f.up(d_roots, io->roots, (size_t)k * sizeof(uint32_t));
  uint32_t launches = 0;
  uint64_t work = 0;
  if (f.rc == POW_OK && io->mode == 0u) f.step(pow_queue_pool_tips(ctx->stream, F, fin, io->flags), "K14a, K14b, K12c, K12d, K14c");
  if (f.rc == POW_OK && io->mode) {
    const PowLiftView v{F.parent, F.depth[fin], d_up, n32, n32, pow_pool_rounds(n32)};
    f.step(pow_queue_pool_lift(ctx->stream, F.parent, d_up, n32, 0, n32, true, &launches, &work), "K13a");
    if (f.rc == POW_OK) f.step(pow_queue_pool_above(ctx->stream, F, fin, v, d_roots, k, d_acc, true, io->mode == 2u), "K14d, K12c, K12d");
    f.down(acc.data(), d_acc, (size_t)k * sizeof(PowAboveAcc));
  }
  f.down(&ctl, F.ctl, sizeof ctl), f.down(io->marks, F.depth[fin ^ 1u], n);
  // the list comes down whole: what lies past the total is scratch, and the caller's array has room for n
  if (io->mode == 0u) f.down(io->list, F.next[0], words);
  if (f.wait("pow_test_pool_above", 100ull * (work + (uint64_t)n32 * (k + 5ull))) != POW_OK) return f.rc;
  const uint32_t kept = ctl.marked;
  if (kept > n32) return fail(POW_EHIP, "K12d counted %u marks on %u nodes", kept, n32);
  if (io->total) *io->total = kept;
  for (uint32_t q = 0; q < k; ++q) {
    if (io->size) io->size[q] = acc[q].size;
    if (io->height) io->height[q] = acc[q].height;
    if (io->best) io->best[q] = acc[q].best;
  }
  if (io->mode != 2u) return POW_OK;
  if (kept >= n32) return fail(POW_EHIP, "K14d kept all %u nodes under %u roots", n32, k);  // a root is a member of its own subtree
  return compact_half(f, "pow_test_pool_above (gather)", F, kept, fin, io->map, io->parent_out, io->depth_out,
                      [](const PowPoolDev&) {});
}

