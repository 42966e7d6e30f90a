// K12  the kernels of pow_pool_mark and pow_pool_prune: every ancestor of a set
// of seed blocks is marked on the device, and a prune compacts the pool's
// resident arrays onto the marked blocks.  Nothing is hashed again and no
// struct goes up: parent, depth, n_bad and the digests are all there (K10,
// K11).  The pool holds n blocks; a prune keeps `kept` of them, in their order.
//
//   K12a pow_pool_prune_seed_kernel    one lane per block, then one per tip.
//        A block's lane starts its walk (next = parent), writes its own
//        position (the map of a prune that drops nothing) and sets its mark if
//        the index rule makes it a seed; a tip's lane sets the mark of the
//        block it names.  The marks were zeroed by the host before the launch,
//        so every store of the launch writes a 1.
//   K12b pow_pool_prune_round_kernel   K10d's pointer jumping with a mark
//        riding along, ceil(log2 n) times, ping-pong on next.
//   K12c pow_pool_prune_count_kernel   the marked blocks of every 256
//        positions (a workgroup of K12e) into a partial: one wave per partial.
//   K12d pow_pool_prune_scan_kernel    one workgroup: the exclusive scan of at
//        most 4,096 partials in place, and the total into the control words.
//   K12e pow_pool_prune_gather_kernel  a marked block's new position is its
//        workgroup's partial plus its rank inside the workgroup; its entries
//        go into the new arrays at that position, and newpos gets it.
//   K12f pow_pool_prune_remap_kernel   one lane per survivor: its parent by the
//        new positions, then K10e's fork choice and flagged count.
//
// The scratch is what the pool has and does not need between calls: next[0]
// and next[1] (the walks; after the rounds next[0] takes newpos and next[1]
// the partials), depth[1 - fin] (the marks, one byte per block) and
// bad[1 - fin] (the positions K12a wrote).
//
// Memory ordering of K12b.  The marks are bytes written in place by plain
// stores while other lanes of the same launch read them, and that is safe.  A
// mark is only ever set, and only on an ancestor of a seed (the block next[i]
// of a marked block i lies on i's walk), so no launch can mark too much.
// Stores of the same value race harmlessly.  A lane that sees a mark another
// lane of its launch has just set marks another ancestor one round early,
// which the later rounds would have marked anyway.  And no launch marks too
// little: after round k the marks cover every ancestor within 2^(k+1) - 1 steps
// of a seed, since the marks a launch found set at its start (those within
// 2^k - 1 steps) each mark the block 2^k steps along.  That needs every walk of
// a round to jump the same length, which is why next goes ping-pong and is
// never updated in place.  Between launches the stream orders everything.  No
// fence is needed and nobody spins.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pow_ctx.h"

// n blocks and n_tips tips.  flags: POW_KEEP_BY_INDEX, POW_KEEP_SOUND_ONLY.
__global__ __launch_bounds__(256) void pow_pool_prune_seed_kernel(uint32_t n, uint32_t n_tips,
                                                                  const uint32_t* __restrict__ tips,
                                                                  const uint32_t* __restrict__ parent,
                                                                  const uint32_t* __restrict__ index,
                                                                  const uint32_t* __restrict__ bad, uint32_t min_index,
                                                                  uint32_t flags, uint32_t* __restrict__ next,
                                                                  uint32_t* __restrict__ self, uint8_t* mark) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) {
    next[i] = parent[i];
    self[i] = i;
    bool seed = (flags & POW_KEEP_BY_INDEX) && index[i] >= min_index;
    if (seed && (flags & POW_KEEP_SOUND_ONLY)) seed = bad[i] == 0u;
    if (seed) mark[i] = 1;
  } else if (i - n < n_tips) {
    const uint32_t t = tips[i - n];
    if (t < n) mark[t] = 1;  // the host has checked it
  }
}

// One round: a marked block marks the block its walk stands at, then every
// walk that has not ended jumps as K10d's does.
__global__ __launch_bounds__(256) void pow_pool_prune_round_kernel(uint32_t n, const uint32_t* __restrict__ next_a,
                                                                   uint32_t* __restrict__ next_b, uint8_t* mark) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  uint32_t nx = next_a[i];
  if (nx < n) {
    if (mark[i]) mark[nx] = 1;
    nx = next_a[nx];
  }
  next_b[i] = nx;
}

// mark4: the marks four to a word, zero past n (the host's reset covers whole
// words).  Wave w of the launch counts the positions 256 w .. 256 w + 255.
__global__ __launch_bounds__(256) void pow_pool_prune_count_kernel(const uint32_t* __restrict__ mark4, uint32_t words,
                                                                   uint32_t n_part, uint32_t* __restrict__ partial) {
  const uint32_t w = blockIdx.x * 256u + threadIdx.x;  // the word, and 64 words are a partial
  uint32_t c = w < words ? (uint32_t)__builtin_popcount(mark4[w] & 0x01010101u) : 0u;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) c += (uint32_t)__shfl_xor((int)c, off);
  const uint32_t part = w >> 6;
  if ((threadIdx.x & 63u) == 0u && part < n_part) partial[part] = c;
}

// One workgroup.  Lane t takes the partials 16 t .. 16 t + 15 (n_part <= 4,096):
// their sum, the exclusive scan of the 256 sums (a wave's by shuffles, the four
// waves' through LDS), and each partial becomes the sum of those before it.
__global__ __launch_bounds__(256) void pow_pool_prune_scan_kernel(uint32_t* __restrict__ partial, uint32_t n_part,
                                                                  PowPoolLiveCtl* ctl) {
  __shared__ uint32_t wave_sum[4];
  const uint32_t t = threadIdx.x, lane = t & 63u, first = 16u * t;
  uint32_t v[16], sum = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    v[k] = first + k < n_part ? partial[first + k] : 0u;
    sum += v[k];
  }
  uint32_t incl = sum;
#pragma unroll
  for (int off = 1; off <= 32; off <<= 1) {
    const uint32_t up = (uint32_t)__shfl_up((int)incl, off);
    if (lane >= (uint32_t)off) incl += up;
  }
  if (lane == 63u) wave_sum[t >> 6] = incl;
  __syncthreads();
  uint32_t before = incl - sum, total = 0;
#pragma unroll
  for (uint32_t w = 0; w < 4; ++w) {
    const uint32_t s = wave_sum[w];
    if (w < (t >> 6)) before += s;
    total += s;
  }
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    if (first + k < n_part) partial[first + k] = before;
    before += v[k];
  }
  if (t == 0) ctl->marked = total;  // the marked blocks of the pool
}

// From the arrays F (n blocks, the final depth and n_bad in depth_f, bad_f)
// into the arrays T (room for cap blocks), out of place: in place a block
// would land on one that has not been read yet.  The parent goes over as it
// is; K12f renames it once every newpos stands.
__global__ __launch_bounds__(256) void pow_pool_prune_gather_kernel(
    uint32_t n, uint32_t cap, const uint8_t* __restrict__ mark, const uint32_t* __restrict__ partial,
    const uint4* __restrict__ dig_f, const uint4* __restrict__ prev_f, const uint32_t* __restrict__ index_f,
    const uint32_t* __restrict__ parent_f, const uint32_t* __restrict__ depth_f, const uint32_t* __restrict__ bad_f,
    const uint8_t* __restrict__ status_f, const uint8_t* __restrict__ kind_f, uint4* __restrict__ dig_t,
    uint4* __restrict__ prev_t, uint32_t* __restrict__ index_t, uint32_t* __restrict__ parent_t,
    uint32_t* __restrict__ depth_t, uint32_t* __restrict__ bad_t, uint8_t* __restrict__ status_t,
    uint8_t* __restrict__ kind_t, uint32_t* __restrict__ newpos) {
  __shared__ uint32_t wave_count[4];
  const uint32_t i = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const bool on = i < n && mark[i] != 0;
  const unsigned long long vote = __ballot(on);
  if (lane == 0u) wave_count[wave] = (uint32_t)__builtin_popcountll(vote);
  __syncthreads();
  uint32_t j = partial[blockIdx.x] + (uint32_t)__builtin_popcountll(vote & ((1ull << lane) - 1ull));
#pragma unroll
  for (uint32_t w = 0; w < 3; ++w)
    if (w < wave) j += wave_count[w];
  if (i >= n) return;
  const bool keep = on && j < cap;  // j < kept <= cap: the count, the scan and this launch read the same marks
  newpos[i] = keep ? j : POW_POOL_NONE;
  if (!keep) return;
  dig_t[2u * j] = dig_f[2u * i];
  dig_t[2u * j + 1u] = dig_f[2u * i + 1u];
  prev_t[2u * j] = prev_f[2u * i];
  prev_t[2u * j + 1u] = prev_f[2u * i + 1u];
  index_t[j] = index_f[i];
  parent_t[j] = parent_f[i];
  depth_t[j] = depth_f[i];
  bad_t[j] = bad_f[i];
  status_t[j] = status_f[i];
  kind_t[j] = kind_f[i];
}

// One lane per survivor (kept of them; n: the blocks before the prune, whose
// newpos this reads).  A parent that is a block is kept, since the marked set
// is closed under parent; POW_POOL_ROOT and POW_POOL_NONE stay.  Then K10e's
// wave reduction into the new arrays' control words, which the host zeroed.
__global__ __launch_bounds__(256) void pow_pool_prune_remap_kernel(uint32_t kept, uint32_t n,
                                                                   const uint32_t* __restrict__ newpos,
                                                                   uint32_t* __restrict__ parent,
                                                                   const uint32_t* __restrict__ bad,
                                                                   const uint8_t* __restrict__ status,
                                                                   const uint32_t* __restrict__ index,
                                                                   PowPoolCtl* ctl) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  unsigned long long key = 0ull;
  bool flagged = false;
  if (j < kept) {
    const uint32_t par = parent[j];
    if (par < n) parent[j] = newpos[par];
    if (bad[j] == 0u) key = ((unsigned long long)index[j] << 32) | (uint32_t)~j;
    flagged = status[j] != 0u;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)key, off);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(key >> 32), off);
    const unsigned long long other = ((unsigned long long)hi << 32) | lo;
    key = other > key ? other : key;
  }
  const unsigned long long any = __ballot(flagged);
  if ((threadIdx.x & 63u) == 0u) {
    if (key) atomicMax(&ctl->best, key);
    if (any) atomicAdd(&ctl->n_flagged, (uint32_t)__builtin_popcountll(any));
  }
}

// D: the pool's arrays with D.n blocks; fin: which of depth[], bad[] are final.
// The marks lie in depth[1 - fin], the positions in bad[1 - fin], the first
// state of the walks in next[0].
hipError_t pow_launch_pool_prune_seed(hipStream_t stream, const PowPoolDev& D, uint32_t fin, const uint32_t* tips,
                                      uint32_t n_tips, uint32_t min_index, uint32_t flags) {
  hipLaunchKernelGGL(pow_pool_prune_seed_kernel, dim3((D.n + n_tips + 255u) / 256u), dim3(256), 0, stream, D.n, n_tips,
                     tips, D.parent, D.index, D.bad[fin], min_index, flags, D.next[0], D.bad[fin ^ 1u],
                     (uint8_t*)D.depth[fin ^ 1u]);
  return hipGetLastError();
}

// Round r reads next[r & 1] and writes the other.
hipError_t pow_launch_pool_prune_round(hipStream_t stream, const PowPoolDev& D, uint32_t fin, uint32_t r) {
  const uint32_t a = r & 1u;
  hipLaunchKernelGGL(pow_pool_prune_round_kernel, dim3((D.n + 255u) / 256u), dim3(256), 0, stream, D.n, D.next[a],
                     D.next[a ^ 1u], (uint8_t*)D.depth[fin ^ 1u]);
  return hipGetLastError();
}

// After the rounds: the partials into next[1].
hipError_t pow_launch_pool_prune_count(hipStream_t stream, const PowPoolDev& D, uint32_t fin) {
  const uint32_t words = (D.n + 3u) / 4u, n_part = (D.n + 255u) / 256u;
  hipLaunchKernelGGL(pow_pool_prune_count_kernel, dim3((words + 255u) / 256u), dim3(256), 0, stream,
                     (const uint32_t*)D.depth[fin ^ 1u], words, n_part, D.next[1]);
  return hipGetLastError();
}

hipError_t pow_launch_pool_prune_scan(hipStream_t stream, const PowPoolDev& D) {
  hipLaunchKernelGGL(pow_pool_prune_scan_kernel, dim3(1), dim3(256), 0, stream, D.next[1], (D.n + 255u) / 256u,
                     (PowPoolLiveCtl*)D.ctl);
  return hipGetLastError();
}

// From the pool's arrays F into T, whose capacity is cap; newpos into F's next[0].
hipError_t pow_launch_pool_prune_gather(hipStream_t stream, const PowPoolDev& F, const PowPoolDev& T, uint32_t cap,
                                        uint32_t fin) {
  hipLaunchKernelGGL(pow_pool_prune_gather_kernel, dim3((F.n + 255u) / 256u), dim3(256), 0, stream, F.n, cap,
                     (const uint8_t*)F.depth[fin ^ 1u], F.next[1], (const uint4*)F.dig, (const uint4*)F.prev, F.index,
                     F.parent, F.depth[fin], F.bad[fin], F.status, F.kind, (uint4*)T.dig, (uint4*)T.prev, T.index,
                     T.parent, T.depth[fin], T.bad[fin], T.status, T.kind, F.next[0]);
  return hipGetLastError();
}

// T.n: the survivors; F.n: the blocks before the prune.
hipError_t pow_launch_pool_prune_remap(hipStream_t stream, const PowPoolDev& F, const PowPoolDev& T, uint32_t fin) {
  hipLaunchKernelGGL(pow_pool_prune_remap_kernel, dim3((T.n + 255u) / 256u), dim3(256), 0, stream, T.n, F.n, F.next[0],
                     T.parent, T.bad[fin], T.status, T.index, T.ctl);
  return hipGetLastError();
}
