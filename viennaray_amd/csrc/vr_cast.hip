// vr_cast.hip — closest-hit queries for the caller's rays (vr_cast_rays_device; include/viennaray_amd.h has the
// definition, vr_cast.hpp the per-ray bookkeeping, vr_cast_rays.cpp the host side).  A translation unit of its own:
// nothing an apply() runs is in it.
//
//   cast_rays_kernel<GEO, D>   a persistent grid.  Every wave owns, for its whole life, one slab of the walk's global
//                              stack (p.walkStack: VR_STACK_GLOBAL * 64 words per wave) and its lanes' columns of the
//                              block's LDS stack ([entry][lane], VR_STACK_LDS entries), and takes groups of 64 rays in a
//                              grid-stride loop.  The launcher never starts more waves than there are slabs or groups.
//
// A ray is what the tracer makes of a host ray (vr_set_host_rays): the origin as given, the direction as given —
// NOT normalised — except that in 2-D a direction with z != 0 has z dropped and is then normalised (project_dir<2>,
// rayUtil.hpp:204-215).  t therefore runs in units of the direction's length wherever the direction is used as it stands
// (3-D; 2-D with z == 0), which is what Trace.occluded relies on.
//
// A segment is the tracer's: pair_walk_lanes over the pair nodes, then hit_walls, the tie rule min t / boundary first /
// lower original id.  A geometry hit ends the ray; a wall continues it through process_boundary_hit<D> from the new
// origin with the tracer's tnear (1e-4), as trace_kernel does.  Why the per-lane pair walk and not a packet path: the
// caller's rays share neither a source plane nor a sort bin, which is what the packet walk, the packet query, the lattice
// table and the LDS small-scene kernel are built on; the pair walk is the one walk that is right for any ray, and the one
// tests/test_edge_rays.py holds to the brute force bit for bit.
//
// Order.  The rays of a group are read through the optional permutation (the host sorts ray indices by the Morton key of
// the origins): one scattered 24-byte gather per ray, issued once, before the loop.  Results go to the caller's rows.
#include <hip/hip_runtime.h>

#include "vr_cast.hpp"
#include "vr_kernels.hpp"
#include "vr_trace_kernel.hpp"

namespace vr {

constexpr float VR_CAST_TNEAR_NEXT = 1e-4f; // tnear of every segment after the first: the tracer's

template <int GEO, int D>
__global__ __launch_bounds__(VR_BLOCK) void cast_rays_kernel(const TraceParams p, const CastArgs a) {
  __shared__ float wallS[VR_WALL_TABLE];
  __shared__ unsigned stackS[VR_STACK_LDS * VR_BLOCK]; // [entry][thread of the block]: entry e of a lane at stackS[e * VR_BLOCK]
  for (unsigned k = threadIdx.x; k < VR_WALL_TABLE; k += blockDim.x)
    wallS[k] = p.wallTable[k];
  __syncthreads(); // (the only block-wide point: from here on the waves run on their own)
  const unsigned lane = threadIdx.x & 63u;
  const unsigned wavesPerBlock = blockDim.x >> 6;
  const unsigned wave = blockIdx.x * wavesPerBlock + (threadIdx.x >> 6); // < waves <= the slabs of p.walkStack (launch_cast_rays)
  const unsigned waves = gridDim.x * wavesPerBlock;
  unsigned *const stackL = stackS + threadIdx.x;
  unsigned *const stackG = p.walkStack + (size_t)wave * (VR_STACK_GLOBAL * 64u) + lane;
  const uint4 *__restrict__ pnodes = reinterpret_cast<const uint4 *>(p.pnodes);
  const float4 *__restrict__ prims = reinterpret_cast<const float4 *>(p.prims);
  const bool follow = (a.flags & 1u) != 0u;
  const float QNAN = __int_as_float(0x7FC00000);
#ifdef VR_DIAG
  unsigned long long phaseDummy[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tLast = 0ull;
  unsigned long long *const phaseT = phaseDummy;
#endif
  VR_DIAG_DECL
  for (unsigned g = wave; g < a.groups; g += waves) {
    const u64 t = (u64)g * 64u + lane;
    const bool valid = t < (u64)a.m;
    // ---- the group's rays: the scattered gather, once ----
    size_t row = 0;
    V3 org = mk(0.f, 0.f, 0.f), rayDirection = mk(0.f, 0.f, 1.f); // (a lane without a ray: harmless values, never walked)
    if (valid) {
      row = a.perm ? (size_t)a.perm[t] : (size_t)t;
      const float *o = a.org + row * a.ld, *d = a.dir + row * a.ld;
      org = mk(o[0], o[1], a.ld == 3u ? o[2] : 0.f);
      rayDirection = mk(d[0], d[1], a.ld == 3u ? d[2] : 0.f);
    }
    V3 dir = project_dir<D>(rayDirection);
    CastState s;
    cast_begin(s);
    V3 hitPoint = mk(QNAN, QNAN, QNAN);
    float tnear = a.tnear;
    bool active = valid;
    // ---- segments, until every ray of the group has ended ----
    while (ballot64(active)) {
      HitRec h;
      hit_clear(h);
      unsigned node = 0u, sp = 0u;
      // (the walk votes wave-wide: every lane takes part in the call, the ended ones with part = false)
      pair_walk_lanes<GEO, VR_STACK_LDS>(p, pnodes, prims, stackL, stackG, active, org, dir, tnear, h, node, sp, 1u VR_DIAG_PASS);
      if (active) {
        hit_walls(p, wallS, org, dir, tnear, h);
        if (h.geom >= 0)
          hitPoint = mk(org.x + dir.x * h.t, org.y + dir.y * h.t, org.z + dir.z * h.t);
        if (cast_segment(s, h.geom, h.prim, h.t, follow, a.maxBoundaryHits, a.tmax) == CAST_AT_WALL) {
          process_boundary_hit<D>(p, wallS, h.prim, hitPoint, org, rayDirection, dir, active);
          if (!active)
            cast_ignored(s);
          tnear = VR_CAST_TNEAR_NEXT;
        } else {
          active = false;
        }
      }
    }
    // ---- results, to the caller's rows ----
    if (valid) {
      int32_t prim;
      float dist;
      uint32_t bh;
      bool hit;
      cast_finish(s, a.tmax, prim, dist, bh, hit);
      a.prim[row] = prim;
      a.dist[row] = dist;
      if (a.hit) {
        a.hit[3 * row] = hit ? hitPoint.x : QNAN;
        a.hit[3 * row + 1] = hit ? hitPoint.y : QNAN;
        a.hit[3 * row + 2] = hit ? hitPoint.z : QNAN;
      }
      if (a.bh)
        a.bh[row] = bh;
    }
  }
}

static unsigned cast_waves(const CastArgs &a, unsigned slabs) {
  // no more waves than slabs, no more than groups; whole blocks of VR_BLOCK / 64 waves once there are that many groups
  const unsigned perBlock = VR_BLOCK / 64;
  unsigned waves = a.groups < slabs ? a.groups : slabs;
  if (waves > perBlock)
    waves -= waves % perBlock;
  return waves;
}

hipError_t launch_cast_rays(const TraceParams &p, int geo, int D, const CastArgs &a, unsigned slabs, hipStream_t st) {
  const unsigned waves = cast_waves(a, slabs);
  if (waves == 0)
    return hipSuccess;
  const unsigned perBlock = VR_BLOCK / 64;
  const dim3 g(waves > perBlock ? waves / perBlock : 1u), b(waves > perBlock ? (unsigned)VR_BLOCK : waves * 64u);
  if (geo == 0) {
    if (D == 2)
      hipLaunchKernelGGL((cast_rays_kernel<0, 2>), g, b, 0, st, p, a);
    else
      hipLaunchKernelGGL((cast_rays_kernel<0, 3>), g, b, 0, st, p, a);
  } else {
    if (D == 2)
      hipLaunchKernelGGL((cast_rays_kernel<1, 2>), g, b, 0, st, p, a);
    else
      hipLaunchKernelGGL((cast_rays_kernel<1, 3>), g, b, 0, st, p, a);
  }
  return hipGetLastError();
}

} // namespace vr
