// Test-library kernels (libpow_gpu_test.so only; build.py TEST_ONLY).
//
// pow_test_stall: one wave that keeps the stream busy for a bounded time
// (POW_TEST_STALL_US), launched in front of a context's next kernel so that
// the host's wait for that kernel outlasts a short watchdog deadline
// (POW_WATCHDOG_MS): the watchdog tests of the HIP launch path.  The wave
// sleeps between reads of the constant-rate realtime counter and always ends.
//
// pow_test_lz: sha256_dev.h's leading_zero_bits (the proof-of-work test of K1,
// K1' and K3 above 32 bits) on digests the caller chooses, one lane each: no
// minable digest reaches its second word's zero branch or any word behind it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sha256_dev.h"

__global__ __launch_bounds__(64) void pow_test_stall(unsigned long long ticks) {
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(127);
}

// us: stall time in microseconds, at most 5 s; realtime_khz: the counter's rate.
extern "C++" hipError_t pow_launch_test_stall(hipStream_t stream, unsigned us, int realtime_khz) {
  const unsigned long long capped = us > 5000000u ? 5000000u : us;
  hipLaunchKernelGGL(pow_test_stall, dim3(1), dim3(64), 0, stream, capped * (unsigned long long)realtime_khz / 1000ull);
  return hipGetLastError();
}

// digests: n x 8 words, most significant first; out: n counts (0..256).
__global__ __launch_bounds__(64) void pow_test_lz(const uint32_t* __restrict__ digests, uint32_t n,
                                                  uint32_t* __restrict__ out) {
  const uint32_t g = blockIdx.x * 64u + threadIdx.x;
  if (g >= n) return;
  uint32_t H[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) H[k] = digests[8u * g + k];
  out[g] = powdev::leading_zero_bits(H);
}

extern "C++" hipError_t pow_launch_test_lz(hipStream_t stream, const uint32_t* digests, uint32_t n, uint32_t* out) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(pow_test_lz, dim3((n + 63u) / 64u), dim3(64), 0, stream, digests, n, out);
  return hipGetLastError();
}
