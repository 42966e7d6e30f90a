// K14  the per-lane test of the pool's descendant queries (pow_pool_subtrees,
// pow_pool_drop): is block r on the walk from block i along parent?  An inline
// function over K13's table (pow_lift_dev.h): the subtree kernel of
// pow_pool_above.hip runs it on the device, and a host compiler takes it as it
// is, so the same code runs on the CPU under sanitizers
// (tests/pool_above_plan_unit.cpp).
//
// If r lies on i's walk it lies depth[i] - depth[r] steps along it, since a
// step along parent takes exactly one off the depth; so one jump of that length
// and one comparison decide it.  A block that is not deeper than r and is not r
// cannot have r under it: with depth[i] < depth[r] the answer is no from the two
// depths alone, and nothing else is read.  That is most lanes of a launch
// whose root stands high in the tree.  The jump's loop has pow_lift_jump's
// constant bound and compares every position it reads with size.
#pragma once
#include <stdint.h>

#include "pow_lift_dev.h"

// i, r < v.size.  r itself is a member of its subtree.
POW_LIFT_FN bool pow_above_member(const PowLiftView& v, uint32_t i, uint32_t r) {
  const uint32_t di = v.depth[i], dr = v.depth[r];
  return di >= dr && pow_lift_jump(v, i, di - dr) == r;
}
