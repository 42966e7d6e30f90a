// What K10 (pow_pool.hip) and K11 (pow_pool_live.hip) share on the device: the
// table's empty slot, the inverse of a name's text and the digest compare of a
// probe.  The probe loops themselves stand in the kernels, where the build
// guards read them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pow_audit_dev.h"

namespace {

constexpr uint32_t SLOT_EMPTY = 0xFFFFFFFFu;

// Four lowercase hex characters (the first in the lowest byte) -> their 16-bit
// value, the first character highest: hex_of16's inverse.  bad collects what
// differs from the text of that value: any byte outside 0-9a-f.
__device__ __forceinline__ uint32_t unhex4(uint32_t t, uint32_t& bad) {
  const uint32_t nib = ((t & 0x0F0F0F0Fu) + ((t >> 6) & 0x01010101u) * 9u) & 0x0F0F0F0Fu;
  bad |= powaudit::hex4(nib) ^ t;
  return ((nib & 0xFu) << 12) | (nib & 0xF00u) | ((nib >> 12) & 0xF0u) | (nib >> 24);
}

__device__ __forceinline__ bool same_digest(const uint4* __restrict__ dig, uint32_t pos, const uint4& a, const uint4& b) {
  const uint4 x = dig[2u * pos], y = dig[2u * pos + 1u];
  return ((x.x ^ a.x) | (x.y ^ a.y) | (x.z ^ a.z) | (x.w ^ a.w) | (y.x ^ b.x) | (y.y ^ b.y) | (y.z ^ b.z) |
          (y.w ^ b.w)) == 0u;
}

}  // namespace
