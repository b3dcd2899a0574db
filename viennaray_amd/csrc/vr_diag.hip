// vr_diag.hip — the diagnostic kernels behind the vr_debug_* entry points (vr_debug.cpp) and their launchers: the
// device functions of the generator and the tracer, run on the caller's inputs so that tests can compare them with the
// reference's known answers one call at a time.
#include <hip/hip_runtime.h>

#include "vr_generate.hpp"
#include "vr_kernels.hpp"
#include "vr_trace_kernel.hpp"

namespace vr {

// vr_debug_surface_source_sample: what the generator's sample gives for the ray indices p.idxList[]
__global__ __launch_bounds__(VR_BLOCK) void debug_surface_kernel(const TraceParams p, float *org, float *dir, float *weight,
                                                                 unsigned *draws) {
  for (unsigned i = blockIdx.x * VR_BLOCK + threadIdx.x; i < p.batchCount; i += gridDim.x * VR_BLOCK) {
    V3 o, d;
    float w;
    u64 lo, hi;
    surface_sample(p, (unsigned)p.idxList[i], o, d, w, lo, hi);
    org[3 * (size_t)i] = o.x;
    org[3 * (size_t)i + 1] = o.y;
    org[3 * (size_t)i + 2] = o.z;
    dir[3 * (size_t)i] = d.x;
    dir[3 * (size_t)i + 1] = d.y;
    dir[3 * (size_t)i + 2] = d.z;
    weight[i] = w;
    draws[i] = 2u;
  }
}

hipError_t launch_debug_surface_sample(const TraceParams &p, unsigned maxBlocks, float *org, float *dir, float *weight,
                                       unsigned *draws, hipStream_t s) {
  unsigned grid = (p.batchCount + VR_BLOCK - 1) / VR_BLOCK;
  if (grid > maxBlocks)
    grid = maxBlocks;
  if (grid)
    hipLaunchKernelGGL(debug_surface_kernel, dim3(grid), dim3(VR_BLOCK), 0, s, p, org, dir, weight, draws);
  return hipGetLastError();
}

template <int GEO>
__global__ void debug_intersect_kernel(const TraceParams p, const float *org, const float *dir, const float *tnear,
                                       unsigned n, int *geomID, unsigned *primID, float *t, int ordered,
                                       unsigned walkStackWaves) {
  __shared__ float wallS[VR_WALL_TABLE];
  __shared__ unsigned stackS[VR_STACK_LDS * VR_BLOCK]; // (64-thread blocks: lane columns 0..63 of the [entry][VR_BLOCK] layout)
  for (unsigned k = threadIdx.x; k < VR_WALL_TABLE; k += blockDim.x)
    wallS[k] = p.wallTable[k];
  __syncthreads();
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  // (the walk votes wave-wide: every lane of the block takes part in the call)
  const unsigned j = i < n ? i : 0u;
  const V3 o = mk(org[3 * j], org[3 * j + 1], org[3 * j + 2]), d = mk(dir[3 * j], dir[3 * j + 1], dir[3 * j + 2]);
  HitRec h;
  hit_clear(h);
#ifdef VR_DIAG
  unsigned long long phaseDummy[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tLast = 0ull;
  unsigned long long *const phaseT = phaseDummy;
#endif
  if (ordered) {
    unsigned node = 0u, sp = 0u;
    VR_DIAG_DECL
    // (diagnostic launches are small: the block index serves as the wave index of the global slab; the host bounds it)
    pair_walk_lanes<GEO, VR_STACK_LDS>(p, reinterpret_cast<const uint4 *>(p.pnodes), reinterpret_cast<const float4 *>(p.prims),
                                       stackS + threadIdx.x, p.walkStack + (size_t)(blockIdx.x % walkStackWaves) * (VR_STACK_GLOBAL * 64u) + threadIdx.x,
                             i < n, o, d, tnear[j], h, node, sp, 1u VR_DIAG_PASS);
  } else {
    unsigned node = 0u;
    VR_DIAG_DECL
    bvh_walk_lanes<GEO>(p, i < n, o, d, tnear[j], h, node, 1u VR_DIAG_PASS);
  }
  hit_walls(p, wallS, o, d, tnear[j], h);
  if (i >= n)
    return;
  geomID[i] = h.geom;
  primID[i] = h.prim;
  t[i] = h.t;
}

hipError_t launch_debug_intersect(const TraceParams &p, int geo, const float *org, const float *dir,
                                  const float *tnear, unsigned n, int *geomID, unsigned *primID, float *t, int ordered,
                                  unsigned walkStackWaves, hipStream_t s) {
  const unsigned grid = (n + 63) / 64;
  if (geo == 0)
    hipLaunchKernelGGL((debug_intersect_kernel<0>), dim3(grid), dim3(64), 0, s, p, org, dir, tnear, n, geomID, primID, t,
                       ordered, walkStackWaves);
  else
    hipLaunchKernelGGL((debug_intersect_kernel<1>), dim3(grid), dim3(64), 0, s, p, org, dir, tnear, n, geomID, primID, t,
                       ordered, walkStackWaves);
  return hipGetLastError();
}

template <int D>
__global__ void debug_process_hit_kernel(const TraceParams p, const float *org, const float *dir, const float *tfar,
                                         const unsigned *prim, unsigned n, float *outOrg, float *outDir, int *outReflect) {
  __shared__ float wallS[VR_WALL_TABLE];
  for (unsigned k = threadIdx.x; k < VR_WALL_TABLE; k += blockDim.x)
    wallS[k] = p.wallTable[k];
  __syncthreads();
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  V3 o = mk(org[3 * i], org[3 * i + 1], org[3 * i + 2]);
  V3 rd = mk(dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]);
  V3 d = project_dir<D>(rd);
  const V3 hp = mk(o.x + d.x * tfar[i], o.y + d.y * tfar[i], o.z + d.z * tfar[i]);
  bool active = true;
  process_boundary_hit<D>(p, wallS, prim[i], hp, o, rd, d, active);
  outOrg[3 * i] = o.x;
  outOrg[3 * i + 1] = o.y;
  outOrg[3 * i + 2] = o.z;
  outDir[3 * i] = d.x;
  outDir[3 * i + 1] = d.y;
  outDir[3 * i + 2] = d.z;
  outReflect[i] = active ? 1 : 0;
}

hipError_t launch_debug_process_hit(const TraceParams &p, int D, const float *org, const float *dir, const float *tfar,
                                    const unsigned *prim, unsigned n, float *outOrg, float *outDir, int *outReflect,
                                    hipStream_t s) {
  const unsigned grid = (n + 63) / 64;
  if (D == 2)
    hipLaunchKernelGGL((debug_process_hit_kernel<2>), dim3(grid), dim3(64), 0, s, p, org, dir, tfar, prim, n, outOrg, outDir, outReflect);
  else
    hipLaunchKernelGGL((debug_process_hit_kernel<3>), dim3(grid), dim3(64), 0, s, p, org, dir, tfar, prim, n, outOrg, outDir, outReflect);
  return hipGetLastError();
}

__global__ __launch_bounds__(VR_BLOCK) void debug_rng_kernel(unsigned seed32, unsigned count, u64 *scratch, u64 *out) {
  if (threadIdx.x != 0)
    return;
  Rng rng;
  rng_init(rng, seed32, scratch);
  unsigned t2 = 0;
  for (unsigned i = 0; i < count; ++i)
    out[i] = rng_next(rng, t2);
}

hipError_t launch_debug_rng(unsigned seed32, unsigned count, unsigned long long *scratch, unsigned long long *out,
                            hipStream_t s) {
  hipLaunchKernelGGL(debug_rng_kernel, dim3(1), dim3(VR_BLOCK), 0, s, seed32, count, scratch, out);
  return hipGetLastError();
}

} // namespace vr
