// vr_setup_common.hpp — what the set-up, ingest, field and results kernels share: the 64-bit word and the ordered-uint
// trick.  Private to vr_bvh.hip, vr_sort.hip, vr_fields.hip, vr_ingest.hip, vr_post.hip and vr_map.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace vr {

typedef unsigned long long u64;

// ---------------------------------------------------------------------------
// float <-> order-preserving uint (for atomicMin/Max on floats)
// ---------------------------------------------------------------------------
__device__ __forceinline__ unsigned f2ord(float f) {
  unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline float ord2f(unsigned u) {
  unsigned v = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
#ifdef __HIP_DEVICE_COMPILE__
  return __uint_as_float(v);
#else
  float f;
  __builtin_memcpy(&f, &v, 4);
  return f;
#endif
}

} // namespace vr
