// Shared host-side helpers for libtonal_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include "../../include/tonal_hip.h"

namespace tl {

void set_error(const char* fmt, ...);

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: launch failed: %s", what, hipGetErrorString(e));
    return TL_ELAUNCH;
  }
  return TL_OK;
}

#define TL_REQUIRE(cond, ...)                \
  do {                                       \
    if (!(cond)) {                           \
      tl::set_error(__VA_ARGS__);            \
      return TL_EINVAL;                      \
    }                                        \
  } while (0)

// the member count of a group entry (tl_*_group): the members are a grid dimension
#define TL_REQUIRE_MEMBERS(entry, M) \
  TL_REQUIRE((M) >= 1 && (M) <= 65535, "%s: the number of members M must lie in [1, 65535] (got %d)", entry, M)

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float lrelu(float z, float slope) { return z > 0.f ? z : z * slope; }
__device__ __forceinline__ float sigmoidf_(float v) { return 1.f / (1.f + expf(-v)); }

// counter-based uniform in [0,1): splitmix64 finaliser over (seed, index)
__device__ __forceinline__ float u01(uint64_t seed, uint64_t idx) {
  uint64_t zz = seed + 0x9E3779B97F4A7C15ull * (idx + 1);
  zz = (zz ^ (zz >> 30)) * 0xBF58476D1CE4E5B9ull;
  zz = (zz ^ (zz >> 27)) * 0x94D049BB133111EBull;
  zz ^= zz >> 31;
  return (float)(zz >> 40) * (1.0f / 16777216.0f);
}

}  // namespace tl
