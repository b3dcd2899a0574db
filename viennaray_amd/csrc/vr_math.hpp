// vr_math.hpp — the vector type, wave votes and reductions, LDS pointer types, reflection (gfx950).
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#else
// the host compiler takes the plain vector arithmetic alone — V3, vdot, vnormalize, reflect_specular, project_dir
// (tests/aux/gather_paths.cpp) — and none of the wave-level parts
#include <cmath>
#define __device__
#define __forceinline__ inline
#endif
namespace vr {

struct V3 {
  float x, y, z;
};

__device__ __forceinline__ V3 mk(float x, float y, float z) { return V3{x, y, z}; }
// (the three components as VALUES before the choice: written as a choice between v.x, v.y and v.z the compiler selects an
//  ADDRESS and loads through it — a vector whose component is picked by a run-time axis (rises_clear, relief_clip) then
//  lives in scratch memory for the whole kernel: the general kernels kept the ray direction there, three scratch loads at
//  every use.  Round 4, found by reading the ISA for scratch_ after the vector L1 turned out to be the bound: C4 -7 %,
//  C2 sticking 0.1 -5 %, the headline -3 %, C5 -3 %, trench3D +- 0)
__device__ __forceinline__ float getc(const V3 &v, int a) {
  const float x = v.x, y = v.y, z = v.z;
  return a == 0 ? x : (a == 1 ? y : z);
}
__device__ __forceinline__ void setc(V3 &v, int a, float f) {
  v.x = a == 0 ? f : v.x;
  v.y = a == 1 ? f : v.y;
  v.z = a == 2 ? f : v.z;
}
// ViennaCore DotProduct: sequential accumulation starting from 0
__device__ __forceinline__ float vdot(const V3 &a, const V3 &b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
// Embree SSE2 dot: x + (y + z)
__device__ __forceinline__ float edot(const V3 &a, const V3 &b) { return a.x * b.x + (a.y * b.y + a.z * b.z); }
__device__ __forceinline__ V3 ecross(const V3 &a, const V3 &b) {
  return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ V3 vsub(const V3 &a, const V3 &b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ void vnormalize(V3 &a) {
  float n = sqrtf(vdot(a, a));
  if (n <= 0.f)
    return;
  a.x /= n;
  a.y /= n;
  a.z /= n;
}

typedef unsigned long long u64;

#if defined(__HIPCC__)
// a device address kept as two words of the frame (lo, hi)
__device__ __forceinline__ unsigned long long frame_addr(const float *f, int lo) {
  return ((unsigned long long)__float_as_uint(f[lo + 1]) << 32) | __float_as_uint(f[lo]);
}

// wave-wide vote as a lane mask.  (HIP's __ballot compares a materialised 0/1 value:
// v_cndmask + v_cmp per call; the builtin hands the condition mask through.)
__device__ __forceinline__ unsigned long long ballot64(bool p) { return __builtin_amdgcn_ballot_w64(p); }
// six comparisons of values already in registers as ONE straight line (a chain of && compiles to nested exec-mask branches)
__device__ __forceinline__ bool all6(bool a, bool b, bool c, bool d, bool e, bool f) {
  return ((int)a & (int)b & (int)c & (int)d & (int)e & (int)f) != 0;
}

__device__ __forceinline__ float lane_bcast(float v, int srcLane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), srcLane));
}

// Six wave-wide reductions at once (three minima, three maxima), result in every lane:
// row_shr 1/2/4/8 + row_bcast 15/31 with the DPP modifier fused into v_min / v_max.  The six
// chains are interleaved, so the two wait states a DPP read of a just-written VGPR needs are
// always filled.  Lanes whose DPP source is out of range keep their value (no bound_ctrl).
__device__ __forceinline__ void wave_minmax6(float &a, float &b, float &c, float &d, float &e, float &f) {
#define VR_DPP6(ctrl)                                                                                                  \
  "v_min_f32_dpp %0, %0, %0 " ctrl "\n v_min_f32_dpp %1, %1, %1 " ctrl "\n v_min_f32_dpp %2, %2, %2 " ctrl "\n"        \
  "v_max_f32_dpp %3, %3, %3 " ctrl "\n v_max_f32_dpp %4, %4, %4 " ctrl "\n v_max_f32_dpp %5, %5, %5 " ctrl "\n"
  // (s_nop 4: the compiler does not know that the block begins with DPP reads — a VGPR written by the VALU instruction
  //  just before it needs two wait states before a DPP instruction may read it, a VALU write of EXEC (v_cmpx, v_readlane
  //  into exec) five, and nothing inserts them for inline assembly.  Found when a second call site, scheduled
  //  differently, returned minima of stale registers now and then; five wait states cover both hazards of the gfx9 table)
  asm volatile("s_nop 4\n" VR_DPP6("row_shr:1 row_mask:0xf bank_mask:0xf") VR_DPP6("row_shr:2 row_mask:0xf bank_mask:0xf")
                   VR_DPP6("row_shr:4 row_mask:0xf bank_mask:0xf") VR_DPP6("row_shr:8 row_mask:0xf bank_mask:0xf")
                       VR_DPP6("row_bcast:15 row_mask:0xa bank_mask:0xf") VR_DPP6("row_bcast:31 row_mask:0xc bank_mask:0xf")
               : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f));
#undef VR_DPP6
  a = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a), 63));
  b = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(b), 63));
  c = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c), 63));
  d = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(d), 63));
  e = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(e), 63));
  f = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(f), 63));
}

// ... four of them (two minima, two maxima): every chain's next step stands four instructions behind the last, which
// still fills the two wait states of a DPP read
__device__ __forceinline__ void wave_minmax4(float &a, float &b, float &c, float &d) {
#define VR_DPP4(ctrl)                                                                                                  \
  "v_min_f32_dpp %0, %0, %0 " ctrl "\n v_min_f32_dpp %1, %1, %1 " ctrl "\n"                                             \
  "v_max_f32_dpp %2, %2, %2 " ctrl "\n v_max_f32_dpp %3, %3, %3 " ctrl "\n"
  asm volatile("s_nop 4\n" VR_DPP4("row_shr:1 row_mask:0xf bank_mask:0xf") VR_DPP4("row_shr:2 row_mask:0xf bank_mask:0xf")
                   VR_DPP4("row_shr:4 row_mask:0xf bank_mask:0xf") VR_DPP4("row_shr:8 row_mask:0xf bank_mask:0xf")
                       VR_DPP4("row_bcast:15 row_mask:0xa bank_mask:0xf") VR_DPP4("row_bcast:31 row_mask:0xc bank_mask:0xf")
               : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
#undef VR_DPP4
  a = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a), 63));
  b = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(b), 63));
  c = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(c), 63));
  d = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(d), 63));
}

// Pointers into LDS carry their address space in the type where they are volatile or travel through a struct: address-
// space inference leaves such accesses on GENERIC pointers, i.e. flat_load / flat_store (the slow path to LDS, waiting on
// both memory counters) — the packet query's frontier lists were read and written that way until round 3.
#define VR_LDS __attribute__((address_space(3)))
typedef unsigned U4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ U4 mk_u4(unsigned x, unsigned y, unsigned z, unsigned w) {
  U4 v;
  v.x = x, v.y = y, v.z = z, v.w = w;
  return v;
}
#endif // __HIPCC__

// rayReflection.hpp:13-29
__device__ __forceinline__ V3 reflect_specular(const V3 &dir, const V3 &n) {
  const V3 inv = V3{-dir.x, -dir.y, -dir.z};
  const float f = 2 * vdot(n, inv);
  return V3{f * n.x - inv.x, f * n.y - inv.y, f * n.z - inv.z};
}

// rayUtil.hpp:204-215 (the D==2 projection of fillRayDirection)
template <int D> __device__ __forceinline__ V3 project_dir(V3 d) {
  if (D == 2) {
    if (d.z != 0.f) {
      d.z = 0.f;
      vnormalize(d);
    }
  }
  return d;
}

} // namespace vr
