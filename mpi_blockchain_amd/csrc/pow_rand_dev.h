// The device side of the reference's generator (glibc's TYPE_3 rand(), pow_host.h), shared by K8
// (pow_rand.hip) and K9 (pow_seed.hip).  Moving a state by n draws is a multiplication by x^n mod
// (x^31 - x^28 - 1), and a polynomial c is applied by walking the generator: y += c[i] x (the
// state after i draws), 31 x 31 multiply-adds.
//
// Lane g of a launch's (K9: a seed's) G = 256 x nwg lanes owns runs of T consecutive trials, [p G T
// + g T, + T) in pass p.  The lanes reach their first from the state they share through the two
// tables of pow_rand_tables (of T alone): workgroup w by B's x^(9 T 256 w), cooperatively, then lane
// l by A's x^(9 T l) on its own copy; from the end of a run to the next by the launch's `step`.
#pragma once

#include <hip/hip_runtime.h>

#include "pow_ctx.h"

namespace powrand {

constexpr uint32_t NW = POW_RAND_WORDS;
constexpr uint32_t LANES = 256u;  // of a workgroup, and so the tables': A[i * LANES + l], then B at NW * LANES + w * NW

// A lane's first trial of the launch, and from the end of a run to its next: below 2^27 by the wrappers' bounds.
__device__ __forceinline__ uint32_t first_rel(uint32_t part, uint32_t run) { return (part * LANES + threadIdx.x) * run; }
__device__ __forceinline__ uint32_t hop_of(uint32_t nwg, uint32_t run) { return nwg * LANES * run - run; }

// The workgroup's state xe[0..30] moved by the polynomial c: the 61-word
// extension, then one output word per lane.  On entry the state is visible to
// lane 0; on return the new one to every lane.
__device__ __forceinline__ void group_move(uint32_t (&xe)[2 * NW + 2], const uint32_t* __restrict__ c) {
  const uint32_t tid = threadIdx.x;
  if (tid == 0)
    for (uint32_t k = NW; k < 2u * NW - 1u; ++k) xe[k] = xe[k - NW] + xe[k - 3u];
  __syncthreads();
  uint32_t mine = 0u;
  if (tid < NW)
    for (uint32_t i = 0; i < NW; ++i) mine += c[i] * xe[i + tid];
  __syncthreads();
  if (tid < NW) xe[tid] = mine;
  __syncthreads();
}

// The lane's state moved by the polynomial coef(0..30), with the state and y
// in registers: the 961 multiply-adds read no LDS.
template <class Coef>
__device__ __forceinline__ void apply(uint32_t (&s)[NW], Coef coef) {
  uint32_t x[NW], y[NW];
#pragma unroll
  for (uint32_t j = 0; j < NW; ++j) {
    x[j] = s[j];
    y[j] = 0u;
  }
#pragma unroll 1
  for (uint32_t i = 0; i < NW; ++i) {
    const uint32_t c = coef(i);
#pragma unroll
    for (uint32_t j = 0; j < NW; ++j) y[j] += c * x[j];
    const uint32_t next = x[0] + x[28];  // the window moves on by one draw
#pragma unroll
    for (uint32_t j = 0; j + 1u < NW; ++j) x[j] = x[j + 1u];
    x[NW - 1u] = next;
  }
#pragma unroll
  for (uint32_t j = 0; j < NW; ++j) s[j] = y[j];
}

}  // namespace powrand
