// K14  the kernels of pow_pool_tips, pow_pool_subtrees and pow_pool_drop: the
// questions that look up the tree from a block.  Nothing is hashed and no
// struct goes up: parent, depth, n_bad and index are all there (K10, K11), the
// membership test reads K13's table (pow_above_dev.h over pow_lift_dev.h), and
// the count, the scan and the compaction are K12's.  The pool holds n blocks.
//
//   K14a pow_pool_above_child_kernel    one lane per block: the byte of its
//        parent is set.  The bytes were zeroed by the host before the launch.
//   K14b pow_pool_above_tip_kernel      one lane per block: its own byte
//        becomes "nobody named me, and I pass the filter".
//        (K12c, K12d: the partials and the total.)
//   K14c pow_pool_above_gather_kernel   a marked block's position goes into a
//        list at its workgroup's partial plus its rank inside the workgroup,
//        K12e's ballot and rank; ascending, since rank follows position.
//   K14d pow_pool_above_subtree_kernel  a grid of ceil(n / 256) x k: lane
//        (i, q) asks whether root q lies on i's walk.  Members are counted,
//        their greatest height over the root and K10e's key are reduced over
//        the wave, and one lane per wave adds them into root q's record, which
//        the host zeroed.  A member also stores a byte, whose value is the
//        launch's: 1 into zeroed marks (pow_pool_subtrees' on[]), 0 into marks
//        preset to 1 (the keep-marks of pow_pool_drop).
//
// The scratch is K12's: depth[1 - fin] as bytes (the marks), next[1] (the
// partials) and next[0] (the list of tips).
//
// Memory ordering.  K14a's bytes are only ever set to 1 within the launch, by
// plain stores, and nobody reads them before the launch ends: equal stores race
// harmlessly, as in K12b.  K14b runs behind it on the stream, and every lane
// reads and writes its own byte only.  K14d's byte stores all carry the
// launch's one value, so two roots that share a member race harmlessly too, and
// no lane reads a mark; its records take atomicAdd and atomicMax only, which
// commute, and are read by the host behind the stream's wait.  K14c reads marks
// and partials that earlier launches wrote and every lane writes its own list
// entry.  Between launches the stream orders everything.  No fence is needed
// and nobody spins.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pow_above_dev.h"
#include "pow_ctx.h"

__global__ __launch_bounds__(256) void pow_pool_above_child_kernel(uint32_t n, const uint32_t* __restrict__ parent,
                                                                   uint8_t* has_child) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t par = parent[i];
  if (par < n) has_child[par] = 1;  // POW_POOL_ROOT and POW_POOL_NONE name nobody
}

// In place: has_child[i] becomes the tip mark of block i.  Bytes past n stay zero.
__global__ __launch_bounds__(256) void pow_pool_above_tip_kernel(uint32_t n, uint32_t sound_only,
                                                                 const uint32_t* __restrict__ bad, uint8_t* mark) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  bool tip = mark[i] == 0;
  if (tip && sound_only) tip = bad[i] == 0u;
  mark[i] = tip ? 1 : 0;
}

// room: the entries of list; the count, the scan and this launch read the same marks, so j < total <= n.
__global__ __launch_bounds__(256) void pow_pool_above_gather_kernel(uint32_t n, uint32_t room,
                                                                    const uint8_t* __restrict__ mark,
                                                                    const uint32_t* __restrict__ partial,
                                                                    uint32_t* __restrict__ list) {
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
  if (on && j < room) list[j] = i;
}

// k roots, gridDim.y = k.  mark (may be null): a member's byte takes `value`.
__global__ __launch_bounds__(256) void pow_pool_above_subtree_kernel(PowLiftView v, uint32_t k,
                                                                     const uint32_t* __restrict__ roots,
                                                                     const uint32_t* __restrict__ index,
                                                                     const uint32_t* __restrict__ bad,
                                                                     PowAboveAcc* acc, uint8_t* mark, uint32_t value) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x, q = blockIdx.y;
  const uint32_t r = q < k ? roots[q] : POW_POOL_NONE;  // the host has checked it
  bool member = false;
  uint32_t height = 0;
  unsigned long long key = 0ull;
  if (i < v.size) {
    if (r < v.size && pow_above_member(v, i, r)) {
      member = true;
      height = v.depth[i] - v.depth[r];
      if (bad[i] == 0u) key = ((unsigned long long)index[i] << 32) | (uint32_t)~i;
      if (mark) mark[i] = (uint8_t)value;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const uint32_t h = (uint32_t)__shfl_xor((int)height, off);
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)key, off);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(key >> 32), off);
    const unsigned long long other = ((unsigned long long)hi << 32) | lo;
    height = h > height ? h : height;
    key = other > key ? other : key;
  }
  const unsigned long long vote = __ballot(member);
  if ((threadIdx.x & 63u) == 0u && vote && q < k) {
    atomicAdd(&acc[q].size, (uint32_t)__builtin_popcountll(vote));
    atomicMax(&acc[q].height, height);
    if (key) atomicMax(&acc[q].best, key);
  }
}

static_assert(POW_LIFT_NONE == POW_POOL_NONE, "pow_lift_dev.h");

// D: the pool's arrays with D.n blocks; fin: which of depth[], bad[] are final.
// The bytes lie in depth[1 - fin], zeroed by the host over whole words.
hipError_t pow_launch_pool_above_child(hipStream_t stream, const PowPoolDev& D, uint32_t fin) {
  hipLaunchKernelGGL(pow_pool_above_child_kernel, dim3((D.n + 255u) / 256u), dim3(256), 0, stream, D.n, D.parent,
                     (uint8_t*)D.depth[fin ^ 1u]);
  return hipGetLastError();
}

hipError_t pow_launch_pool_above_tip(hipStream_t stream, const PowPoolDev& D, uint32_t fin, uint32_t sound_only) {
  hipLaunchKernelGGL(pow_pool_above_tip_kernel, dim3((D.n + 255u) / 256u), dim3(256), 0, stream, D.n, sound_only,
                     D.bad[fin], (uint8_t*)D.depth[fin ^ 1u]);
  return hipGetLastError();
}

// The marks of depth[1 - fin] counted: K12c's partials into next[1], K12d's total into the control words.
hipError_t pow_launch_pool_above_count(hipStream_t stream, const PowPoolDev& D, uint32_t fin) {
  const hipError_t e = pow_launch_pool_prune_count(stream, D, fin);
  return e != hipSuccess ? e : pow_launch_pool_prune_scan(stream, D);
}

// After the count: the marked positions into next[0], which has room for D.n.
hipError_t pow_launch_pool_above_gather(hipStream_t stream, const PowPoolDev& D, uint32_t fin) {
  hipLaunchKernelGGL(pow_pool_above_gather_kernel, dim3((D.n + 255u) / 256u), dim3(256), 0, stream, D.n, D.n,
                     (const uint8_t*)D.depth[fin ^ 1u], D.next[1], D.next[0]);
  return hipGetLastError();
}

// v: the table over D's blocks, up to date.  marks: members store `value` into depth[1 - fin].
hipError_t pow_launch_pool_above_subtree(hipStream_t stream, const PowPoolDev& D, uint32_t fin, const PowLiftView& v,
                                         const uint32_t* roots, uint32_t k, PowAboveAcc* acc, bool marks,
                                         uint32_t value) {
  hipLaunchKernelGGL(pow_pool_above_subtree_kernel, dim3((D.n + 255u) / 256u, k), dim3(256), 0, stream, v, k, roots,
                     D.index, D.bad[fin], acc, marks ? (uint8_t*)D.depth[fin ^ 1u] : nullptr, value);
  return hipGetLastError();
}
