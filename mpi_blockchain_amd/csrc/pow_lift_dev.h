// K13  the per-lane walks of the pool's ancestry queries (pow_pool_ancestors,
// pow_pool_fork_points, pow_pool_chain): one entry of a row of the
// binary-lifting table, the ancestor a number of steps along parent, and the
// fork point of two blocks.  Inline functions over plain arrays: the kernels of
// pow_pool_lift.hip run them on the device, and a host compiler takes them as
// they are, so the same code runs on the CPU under sanitizers
// (tests/pool_lift_plan_unit.cpp).
//
// The table.  Level 0 is the pool's parent array.  Row j (j >= 1) is one array
// of `cap` words at up + (j - 1) cap: up[j][i] is the block 2^j steps under i,
// or the walk's end marker (POW_POOL_ROOT, POW_POOL_NONE) once the walk is
// shorter.  A pool of `size` blocks has `levels` = ceil(log2 size) levels, so
// levels - 1 rows.  Levels 0 .. levels - 1 cover step counts up to
// 2^levels - 1, while a walk's depth can equal 2^levels (a flat chain of 2^k
// blocks): a walk to the end therefore applies the bits of depth - 1, which
// gives the walk's last block, and returns that block's parent.
//
// Whatever the arrays hold (a cycle of names is unspecified, as everywhere in
// the pool), every loop has a constant bound and every position read from the
// table is compared with `size` before it is used as an index.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define POW_LIFT_FN __host__ __device__ inline
#else
#define POW_LIFT_FN inline
#endif

#define POW_LIFT_MAX_LEVELS 20u  // ceil(log2 POW_POOL_MAX_BLOCKS)
#define POW_LIFT_NONE 0xFFFFFFFEu  // POW_POOL_NONE (include/pow_gpu.h)

// The table as the walks see it; all of it read only.
struct PowLiftView {
  const uint32_t* parent;  // level 0, size entries
  const uint32_t* depth;   // size entries: the blocks on the walk from i, i included
  const uint32_t* up;      // rows 1 .. levels - 1, cap words each (never read if levels <= 1)
  uint32_t cap;            // words of a row
  uint32_t size;           // blocks of the pool
  uint32_t levels;         // ceil(log2 size), at most POW_LIFT_MAX_LEVELS
};

// Level j of the table (j < levels).
POW_LIFT_FN const uint32_t* pow_lift_level(const PowLiftView& v, uint32_t j) {
  return j ? v.up + (size_t)(j - 1u) * v.cap : v.parent;
}

// One entry of a row: the block two jumps of the previous level under i.
POW_LIFT_FN uint32_t pow_lift_entry(const uint32_t* prev, uint32_t size, uint32_t i) {
  const uint32_t x = prev[i];
  return x < size ? prev[x] : x;
}

// pos moved by the low `levels` bits of s; stops at an end marker.
POW_LIFT_FN uint32_t pow_lift_jump(const PowLiftView& v, uint32_t pos, uint32_t s) {
  for (uint32_t j = 0; j < POW_LIFT_MAX_LEVELS; ++j) {
    if (j >= v.levels || pos >= v.size) break;
    if ((s >> j) & 1u) pos = pow_lift_level(v, j)[pos];
  }
  return pos;
}

// The block `steps` steps along parent from pos (pos < size), or the walk's end.
POW_LIFT_FN uint32_t pow_lift_ancestor(const PowLiftView& v, uint32_t pos, uint32_t steps) {
  const uint32_t d = v.depth[pos];
  if (steps < d) return pow_lift_jump(v, pos, steps);
  const uint32_t last = pow_lift_jump(v, pos, d ? d - 1u : 0u);
  return last < v.size ? v.parent[last] : last;
}

// The fork point of a and b (both < size): the first block on a's walk that
// also lies on b's, or POW_LIFT_NONE; *back_a, *back_b the steps to it, or the
// two depths.  The deeper side is lifted by the depths' difference; at equal
// depth both entries of a level are blocks or both are end markers, so a
// marker never meets a block.
POW_LIFT_FN uint32_t pow_lift_fork(const PowLiftView& v, uint32_t a, uint32_t b, uint32_t* back_a, uint32_t* back_b) {
  const uint32_t da = v.depth[a], db = v.depth[b];
  const uint32_t la = da > db ? da - db : 0u, lb = db > da ? db - da : 0u;
  uint32_t x = pow_lift_jump(v, a, la), y = pow_lift_jump(v, b, lb), steps = 0, at = POW_LIFT_NONE;
  if (x < v.size && y < v.size) {
    if (x == y) {
      at = x;
    } else {
      for (uint32_t k = 0; k < POW_LIFT_MAX_LEVELS; ++k) {
        if (k >= v.levels) break;
        const uint32_t j = v.levels - 1u - k;
        const uint32_t* const row = pow_lift_level(v, j);
        const uint32_t xa = row[x], yb = row[y];
        if (xa < v.size && yb < v.size && xa != yb) x = xa, y = yb, steps += 1u << j;
      }
      const uint32_t px = v.parent[x], py = v.parent[y];
      if (px == py && px < v.size) at = px, steps += 1u;
    }
  }
  const bool found = at != POW_LIFT_NONE;
  *back_a = found ? la + steps : da;
  *back_b = found ? lb + steps : db;
  return at;
}
