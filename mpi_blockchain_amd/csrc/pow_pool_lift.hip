// K13  the kernels of pow_pool_ancestors, pow_pool_fork_points and
// pow_pool_chain: a binary-lifting table over the pool's parent array, and the
// queries that read it.  Nothing is hashed and no struct goes up: parent and
// depth are all there (K10, K11).  The per-lane walks are pow_lift_dev.h's.
//
//   K13a pow_pool_lift_row_kernel       one row over a range of blocks: entry
//        i of row j is two jumps of level j - 1.
//   K13b pow_pool_lift_small_kernel     one workgroup, at most 256 new blocks
//        at the pool's end, every row that exists already, level by level.
//   K13c pow_pool_lift_ancestor_kernel  one lane per query (pos, steps), or
//        with no arrays (tip, lane): the chain call, whose length word lane 0
//        writes.
//   K13d pow_pool_lift_fork_kernel      one lane per pair.
//
// Memory ordering.  K13a needs none: a launch reads level j - 1 and writes row
// j, which are different arrays, level j - 1 was written by earlier launches of
// the stream, and every lane writes its own entry only.
// K13b runs the levels in order inside one launch, and a new block's parent may
// be another new block of the same batch, so a lane needs entries that other
// lanes of its launch make.  Those never travel through global memory: a lane
// keeps its own entry of the previous level in a register and puts it into
// LDS, a barrier follows, and a lane whose jump lands on a new block takes that
// block's entry from LDS; one that lands on an old block reads the old block's
// row, which earlier launches wrote and this launch does not write (it stores
// new blocks' entries only, and nobody reads those from global memory before
// the launch ends).  LDS goes ping-pong by level, so the one barrier of a level
// also separates its reads from the next level's writes to the other half.
// Between launches the stream orders everything.  No fence is needed and nobody
// spins.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pow_ctx.h"
#include "pow_lift_dev.h"

static_assert((1u << POW_LIFT_MAX_LEVELS) == POW_POOL_MAX_BLOCKS && POW_LIFT_NONE == POW_POOL_NONE, "pow_lift_dev.h");

// Blocks first .. first + count - 1 of one row; size: the pool's blocks.
__global__ __launch_bounds__(256) void pow_pool_lift_row_kernel(uint32_t first, uint32_t count, uint32_t size,
                                                                const uint32_t* __restrict__ prev,
                                                                uint32_t* __restrict__ row) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= count || first + t >= size) return;
  row[first + t] = pow_lift_entry(prev, size, first + t);
}

// Blocks first .. size - 1 (at most 256) of rows 1 .. rows; cap: words of a row.
__global__ __launch_bounds__(256) void pow_pool_lift_small_kernel(uint32_t first, uint32_t size, uint32_t rows,
                                                                  uint32_t cap, const uint32_t* __restrict__ parent,
                                                                  uint32_t* up) {
  __shared__ uint32_t hand[2][256];
  const uint32_t t = threadIdx.x, i = first + t;
  const bool on = i < size;
  uint32_t mine = on ? parent[i] : POW_POOL_NONE;  // this lane's entry of the level below
  for (uint32_t j = 1; j < POW_LIFT_MAX_LEVELS; ++j) {
    if (j > rows) break;
    uint32_t* const h = hand[j & 1u];
    h[t] = mine;
    __syncthreads();
    if (mine < size) {
      if (mine >= first) {
        mine = h[(mine - first) & 255u];
      } else {
        const uint32_t* const below = j > 1u ? up + (size_t)(j - 2u) * cap : parent;
        mine = below[mine];
      }
    }
    if (on) up[(size_t)(j - 1u) * cap + i] = mine;
  }
}

// k queries.  pos == nullptr: the chain call, query q is (tip, q); it answers
// POW_POOL_NONE past the walk's length, which lane 0 writes behind the answers.
__global__ __launch_bounds__(256) void pow_pool_lift_ancestor_kernel(PowLiftView v, uint32_t k,
                                                                     const uint32_t* __restrict__ pos,
                                                                     const uint32_t* __restrict__ steps, uint32_t tip,
                                                                     uint32_t* __restrict__ out) {
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  if (q >= k) return;
  if (pos) {
    const uint32_t at = pos[q];
    out[q] = at < v.size ? pow_lift_ancestor(v, at, steps[q]) : POW_POOL_NONE;  // the host has checked it
    return;
  }
  const uint32_t d = tip < v.size ? v.depth[tip] : 0u, len = d < k ? d : k;
  out[q] = q < len ? pow_lift_ancestor(v, tip, q) : POW_POOL_NONE;
  if (q == 0u) out[k] = len;
}

// k pairs: at, back_a and back_b are k words each.
__global__ __launch_bounds__(256) void pow_pool_lift_fork_kernel(PowLiftView v, uint32_t k,
                                                                 const uint32_t* __restrict__ a,
                                                                 const uint32_t* __restrict__ b,
                                                                 uint32_t* __restrict__ at,
                                                                 uint32_t* __restrict__ back_a,
                                                                 uint32_t* __restrict__ back_b) {
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  if (q >= k) return;
  const uint32_t x = a[q], y = b[q];
  uint32_t ba = 0, bb = 0, f = POW_POOL_NONE;
  if (x < v.size && y < v.size) f = pow_lift_fork(v, x, y, &ba, &bb);  // the host has checked them
  at[q] = f;
  back_a[q] = ba;
  back_b[q] = bb;
}

// Row j (1 .. rows) of the table at up, cap words a row, over the blocks
// first .. first + count - 1 of a pool of `size`.
hipError_t pow_launch_pool_lift_row(hipStream_t stream, const uint32_t* parent, uint32_t* up, uint32_t cap, uint32_t j,
                                    uint32_t first, uint32_t count, uint32_t size) {
  const uint32_t* const prev = j > 1u ? up + (size_t)(j - 2u) * cap : parent;
  hipLaunchKernelGGL(pow_pool_lift_row_kernel, dim3((count + 255u) / 256u), dim3(256), 0, stream, first, count, size,
                     prev, up + (size_t)(j - 1u) * cap);
  return hipGetLastError();
}

// Rows 1 .. rows over the blocks first .. size - 1, at most 256 of them.
hipError_t pow_launch_pool_lift_small(hipStream_t stream, const uint32_t* parent, uint32_t* up, uint32_t cap,
                                      uint32_t rows, uint32_t first, uint32_t size) {
  hipLaunchKernelGGL(pow_pool_lift_small_kernel, dim3(1), dim3(256), 0, stream, first, size, rows, cap, parent, up);
  return hipGetLastError();
}

// out: k words, and one more (the length) if pos is null.
hipError_t pow_launch_pool_lift_ancestor(hipStream_t stream, const PowLiftView& v, uint32_t k, const uint32_t* pos,
                                         const uint32_t* steps, uint32_t tip, uint32_t* out) {
  hipLaunchKernelGGL(pow_pool_lift_ancestor_kernel, dim3((k + 255u) / 256u), dim3(256), 0, stream, v, k, pos, steps,
                     tip, out);
  return hipGetLastError();
}

hipError_t pow_launch_pool_lift_fork(hipStream_t stream, const PowLiftView& v, uint32_t k, const uint32_t* a,
                                     const uint32_t* b, uint32_t* at, uint32_t* back_a, uint32_t* back_b) {
  hipLaunchKernelGGL(pow_pool_lift_fork_kernel, dim3((k + 255u) / 256u), dim3(256), 0, stream, v, k, a, b, at, back_a,
                     back_b);
  return hipGetLastError();
}
