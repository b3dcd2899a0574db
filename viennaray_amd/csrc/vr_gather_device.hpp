// vr_gather_device.hpp — the small device functions the gather's kernel files share (vr_gather.hip: gather_samples_kernel;
// vr_gather_species.hip: gather_species_kernel): where a lane's primitive and a hit's normal come from in the packed
// records, the streaming draw of a chunk's engine, and the tnear of every segment.  What a sample IS stays in
// vr_gather.hpp; the walk in vr_cast.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include "vr_cast.hpp"
#include "vr_gather.hpp"
#include "vr_trace_kernel.hpp"

namespace vr {

constexpr float VR_GATHER_TNEAR = 1e-4f; // tnear of every segment: the tracer's

__device__ __forceinline__ V3 v3(const GVec &v) { return V3{v.x, v.y, v.z}; }

// origin o_i and normal m_i of the primitive at leaf position q, and its original id
template <int GEO>
__device__ __forceinline__ void gather_primitive(const float4 *__restrict__ prims, unsigned q, GVec &org, GVec &nrm, unsigned &orig) {
  if (GEO == 0) {
    const float4 c4 = prims[2 * (size_t)q], n4 = prims[2 * (size_t)q + 1];
    org = GVec{c4.x, c4.y, c4.z};
    nrm = GVec{n4.x, n4.y, n4.z};
    orig = __float_as_uint(n4.w);
  } else {
    const float4 a = prims[4 * (size_t)q], b = prims[4 * (size_t)q + 1], c = prims[4 * (size_t)q + 2], e = prims[4 * (size_t)q + 3];
    org = gather_tri_centroid(GVec{a.x, a.y, a.z}, GVec{b.x, b.y, b.z}, GVec{c.x, c.y, c.z});
    nrm = GVec{b.w, c.w, e.w};
    gather_normalize(nrm);
    orig = __float_as_uint(a.w);
  }
}
// the normal the tracer tests a hit's side against (trace_kernel: geomNormal)
template <int GEO> __device__ __forceinline__ V3 gather_hit_normal(const float4 *__restrict__ prims, unsigned q) {
  if (GEO == 0) {
    const float4 n4 = prims[2 * (size_t)q + 1];
    return mk(n4.x, n4.y, n4.z);
  }
  return mk(prims[4 * (size_t)q + 1].w, prims[4 * (size_t)q + 2].w, prims[4 * (size_t)q + 3].w);
}

// the next output of the streaming tier: k < 156 (vr_rng.hpp: rng_next's first branch)
__device__ __forceinline__ u64 gather_draw(unsigned &k, u64 &lo, u64 &hi) {
  const u64 lo1 = mt_step(lo, k + 1u);
  const u64 v = mt_temper(mt_twist(lo, lo1, hi));
  lo = lo1;
  hi = mt_step(hi, k + 157u);
  ++k;
  return v;
}

} // namespace vr
