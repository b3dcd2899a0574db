// vr_intersect.hpp — the primitive tests: disc, triangle, walls, the neighbour-disk test, and their branch-free and
// uniform-disk forms; the closest-hit record (gfx950).
#pragma once
#include "vr_frame.hpp"
#include "vr_math.hpp"
#include "vr_types.hpp"
namespace vr {

// ---------------------------------------------------------------------------
// Primitive tests — Embree 4.3.3 semantics restated
// ---------------------------------------------------------------------------
// oriented disc: plane hit, tnear <= t, dist^2 < r^2
__device__ __forceinline__ bool hit_disc(const V3 &o, const V3 &d, float tnear, const float4 &c4, const V3 &n,
                                         float &tOut) {
  const float divisor = edot(d, n);
  if (divisor == 0.f)
    return false;
  const V3 co = V3{c4.x - o.x, c4.y - o.y, c4.z - o.z};
  const float t = edot(co, n) / divisor;
  if (!(tnear <= t && t <= 3.402823466e+38f))
    return false;
  const V3 p = V3{o.x + d.x * t - c4.x, o.y + d.y * t - c4.y, o.z + d.z * t - c4.z};
  const float dist2 = edot(p, p);
  if (!(dist2 < c4.w * c4.w))
    return false;
  tOut = t;
  return true;
}

__device__ __forceinline__ float xorsign(float v, float s) {
  return __uint_as_float(__float_as_uint(v) ^ (__float_as_uint(s) & 0x80000000u));
}

// Moeller-Trumbore, Embree form: den != 0, U,V >= 0, U+V <= |den|, |den| tnear < T
__device__ __forceinline__ bool hit_tri(const V3 &o, const V3 &d, float tnear, const V3 &v0, const V3 &e1,
                                        const V3 &e2, const V3 &Ng, float &tOut) {
  const V3 C = vsub(v0, o);
  const V3 R = ecross(C, d);
  const float den = edot(Ng, d);
  const float absDen = fabsf(den);
  const float U = xorsign(edot(R, e2), den);
  const float V = xorsign(edot(R, e1), den);
  if (!(den != 0.f && U >= 0.f && V >= 0.f && U + V <= absDen))
    return false;
  const float T = xorsign(edot(Ng, C), den);
  if (!(absDen * tnear < T && T <= absDen * 3.402823466e+38f))
    return false;
  tOut = T / absDen;
  return true;
}

struct HitRec {
  float t;
  int geom;       // -1 miss, 0 boundary, 1 geometry
  unsigned prim;  // wall id, or ORIGINAL primitive id
  unsigned pos;   // leaf position of the geometry primitive
};

// Exact pre-test for an axis-aligned wall at coordinate W on axis a: the
// Moeller-Trumbore depth test can only pass when (W - o_a) and d_a have the
// same strict sign (the other two components of the wall's Ng are exactly 0),
// so walls failing it are skipped without changing any result.
__device__ __forceinline__ bool wall_reachable(float W, float oa, float da) {
  const float c = W - oa;
  return (c > 0.f && da > 0.f) || (c < 0.f && da < 0.f);
}

__device__ __forceinline__ void hit_clear(HitRec &h) {
  h.t = 3.402823466e+38f;
  h.geom = -1;
  h.prim = 0xFFFFFFFFu;
  h.pos = 0;
}

// closest-hit rule: min t; ties -> boundary first, then lower original id
__device__ __forceinline__ bool hit_update(HitRec &h, bool ok, float t, unsigned orig, unsigned q) {
  const bool take = ok && (t < h.t || (t == h.t && h.geom == 1 && orig < h.prim));
  if (take) {
    h.t = t;
    h.geom = 1;
    h.prim = orig;
    h.pos = q;
  }
  return take;
}

// Conservative pre-test of a disc from its first record word {c, r} alone: a ray can only pass
// hit_disc / local_disc_hit if its LINE comes within r of the centre and the disc is not entirely
// behind the origin.  The per-lane paths are bound by the vector memory pipeline (one address per
// clock per CU for scattered gathers), so a disc's second word (normal, id) is only
// fetched by the lanes that pass.  Margins cover the rounding of the cancellation in q (a few ulp
// of |c - o|^2); a pass decides nothing, the exact test follows.
__device__ __forceinline__ bool disc_may_hit(const V3 &o, const V3 &d, float invDD, const float4 &c4) {
  const V3 oc = V3{c4.x - o.x, c4.y - o.y, c4.z - o.z};
  const float oc2 = vdot(oc, oc), b = vdot(oc, d), r2 = c4.w * c4.w;
  const float q = oc2 - b * b * invDD; // squared distance of the centre from the line
  return q <= r2 * 1.001f + 2e-6f * oc2 && !(b < 0.f && oc2 > r2 * 1.01f + 1e-12f);
}

// boundary: 8 wall triangles {v0,e1,e2,Ng} in LDS; pairs (0,1) (2,3) lie on the
// firstDir min/max planes, (4,5) (6,7) on the secondDir min/max planes.
// Called AFTER the geometry walk with the geometry's closest hit in `h`: most rays meet
// the surface long before they could reach a wall plane, and for those the (long)
// triangle tests are skipped.  A wall wins against geometry at equal t (closest-hit rule:
// boundary first); among walls the lower id wins.
template <bool FRAME_LDS>
__device__ __forceinline__ void hit_walls_from(const TraceParams &p, const float *__restrict__ wallS, const V3 &o,
                                               const V3 &d, float tnear, HitRec &h) {
  if (p.debugFlags & 8u)
    return;
  HitRec hw;
  hit_clear(hw);
  const float tLimit = h.t * 1.001f; // (plane t below is approximate: generous margin; inf stays inf)
  const int aRay = FRAME_LDS ? __float_as_int(wallS[VR_F_RAYDIR]) : p.rayDir;
  const int aFirst = FRAME_LDS ? __float_as_int(wallS[VR_F_FIRSTDIR]) : p.firstDir;
  const int aSecond = FRAME_LDS ? __float_as_int(wallS[VR_F_SECONDDIR]) : p.secondDir;
  const float o1 = getc(o, aFirst), d1 = getc(d, aFirst);
  const float o2 = getc(o, aSecond), d2 = getc(d, aSecond);
#pragma unroll
  for (int pair = 0; pair < 4; ++pair) {
    const float *w0 = wallS + 24 * pair;
    // the wall planes are the adjusted bbox faces: scalars, no LDS read needed to cull
    const float W = FRAME_LDS ? wallS[VR_F_LO1 + pair] /* lo1, hi1, lo2, hi2 */
                              : (pair == 0 ? p.lo1 : (pair == 1 ? p.hi1 : (pair == 2 ? p.lo2 : p.hi2)));
    const float oa = pair < 2 ? o1 : o2, da = pair < 2 ? d1 : d2;
    if (!wall_reachable(W, oa, da))
      continue;
    {
      // conservative pre-tests (the approximate reciprocal is fine, the margins are far
      // above its rounding): the plane must come before the geometry hit, and where the
      // ray meets it, it must lie inside the wall's extent along the tracing axis (the
      // walls span the whole adjusted bbox there)
      const float tw = (W - oa) * __builtin_amdgcn_rcpf(da);
      if (tw > tLimit)
        continue;
      const float cr = getc(o, aRay) + getc(d, aRay) * tw;
      if (cr < (FRAME_LDS ? wallS[VR_F_WALL_LO_R] : p.wallLoR) || cr > (FRAME_LDS ? wallS[VR_F_WALL_HI_R] : p.wallHiR))
        continue;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const float *w = w0 + 12 * j;
      float t;
      if (hit_tri(o, d, tnear, mk(w[0], w[1], w[2]), mk(w[3], w[4], w[5]), mk(w[6], w[7], w[8]),
                  mk(w[9], w[10], w[11]), t)) {
        if (t < hw.t) { // ascending wall id: ties keep the lower id
          hw.t = t;
          hw.geom = 0;
          hw.prim = (unsigned)(2 * pair + j);
        }
      }
    }
  }
  if (hw.geom == 0 && hw.t <= h.t)
    h = hw;
}
__device__ __forceinline__ void hit_walls(const TraceParams &p, const float *__restrict__ wallS, const V3 &o,
                                          const V3 &d, float tnear, HitRec &h) {
  hit_walls_from<false>(p, wallS, o, d, tnear, h);
}
// ... the same with the frame read from LDS (vr_frame.hpp says why)
__device__ __forceinline__ void hit_walls_lds(const TraceParams &p, const float *__restrict__ wallS, const V3 &o,
                                              const V3 &d, float tnear, HitRec &h) {
  hit_walls_from<true>(p, wallS, o, d, tnear, h);
}

// rayTraceKernel.hpp:462-507 (neighbour disk test), also returning the distance between the point of impact and the disc
// centre (VIENNARAY_USE_WDIST, rayTraceKernel.hpp:258-296); false leaves dist undefined
__device__ __forceinline__ bool local_disc_hit_dist(const V3 &ro, const V3 &rd, const float4 &c4, const V3 &n,
                                                    float &dist) {
  const float prod = vdot(n, rd);
  if (prod > 0.f)
    return false;
  if (fabsf(prod) < 1e-6f)
    return false;
  const V3 c = V3{c4.x, c4.y, c4.z};
  const float ddneg = vdot(c, n);
  const float tt = (ddneg - vdot(n, ro)) / prod;
  if (tt <= 0.f)
    return false;
  V3 hp = V3{rd.x * tt + ro.x, rd.y * tt + ro.y, rd.z * tt + ro.z};
  hp.x = hp.x - c.x;
  hp.y = hp.y - c.y;
  hp.z = hp.z - c.z;
  dist = sqrtf(vdot(hp, hp));
  return c4.w > dist;
}

// ... for the callers that do not want the distance
__device__ __forceinline__ bool local_disc_hit(const V3 &ro, const V3 &rd, const float4 &c4, const V3 &n) {
  float dist;
  return local_disc_hit_dist(ro, rd, c4, n, dist);
}

// hit_disc / hit_update / local_disc_hit for the candidate loop of the absorbing flat-scene kernel's packet query
// (pq_hit_packet LEAN): the same arithmetic in the same order, every condition evaluated and combined at the end
// instead of a nest of early returns.  Each early return was a divergent branch — saving and restoring the exec mask
// on the CU's one scalar unit, which is what that kernel queues for (profiles/salu_inventory_mode1.md) — and saved
// nothing: a candidate passed the query's box test, so some lane of the wave nearly always goes all the way.
// (A lane that fails an early condition computes on with an infinity or a NaN and is masked out by that condition.)
__device__ __forceinline__ bool hit_disc_lds(const V3 &o, const V3 &d, float tnear, const float4 &c4, const V3 &n,
                                             float &tOut) {
  const float divisor = edot(d, n);
  const V3 co = V3{c4.x - o.x, c4.y - o.y, c4.z - o.z};
  const float t = edot(co, n) / divisor;
  const V3 p = V3{o.x + d.x * t - c4.x, o.y + d.y * t - c4.y, o.z + d.z * t - c4.z};
  const float dist2 = edot(p, p);
  tOut = t;
  return (divisor != 0.f) & (tnear <= t) & (t <= 3.402823466e+38f) & (dist2 < c4.w * c4.w);
}
__device__ __forceinline__ bool hit_update_lds(HitRec &h, bool ok, float t, unsigned orig, unsigned q) {
  const bool take = ok & ((t < h.t) | ((t == h.t) & (h.geom == 1) & (orig < h.prim)));
  h.t = take ? t : h.t;
  h.geom = take ? 1 : h.geom;
  h.prim = take ? orig : h.prim;
  h.pos = take ? q : h.pos;
  return take;
}
__device__ __forceinline__ bool local_disc_hit_lds(const V3 &ro, const V3 &rd, const float4 &c4, const V3 &n) {
  const float prod = vdot(n, rd);
  const V3 c = V3{c4.x, c4.y, c4.z};
  const float ddneg = vdot(c, n);
  const float tt = (ddneg - vdot(n, ro)) / prod;
  V3 hp = V3{rd.x * tt + ro.x, rd.y * tt + ro.y, rd.z * tt + ro.z};
  hp.x = hp.x - c.x;
  hp.y = hp.y - c.y;
  hp.z = hp.z - c.z;
  const float dist = sqrtf(vdot(hp, hp));
  return !(prod > 0.f) & !(fabsf(prod) < 1e-6f) & !(tt <= 0.f) & (c4.w > dist);
}
// hit_disc_lds / local_disc_hit_lds for a cloud whose disks all have the normal n and one radius (pq_hit_packet UNIFORM).
// divisor = edot(d, n), prod = vdot(n, rd) and nro = vdot(n, ro) are the caller's, computed once per ray and round; every
// other operation is the one above, in its order.  thresh is the smallest float x with sqrtf(x) >= radius: the correctly
// rounded square root is monotone, so radius > sqrtf(x) <=> x < thresh for every x (an infinity or a NaN: both false).
// (Where the disks share a plane normal to a coordinate axis as well, t, tt and the two points are the ray's too:
//  vr_planar_disks.hpp has those forms, pq_hit_packet PLANAR uses them in place of these two.)
__device__ __forceinline__ bool hit_disc_uniform(const V3 &o, const V3 &d, float tnear, const V3 &c, const V3 &n, float divisor,
                                                 float radius, float &tOut) {
  const V3 co = V3{c.x - o.x, c.y - o.y, c.z - o.z};
  const float t = edot(co, n) / divisor;
  const V3 p = V3{o.x + d.x * t - c.x, o.y + d.y * t - c.y, o.z + d.z * t - c.z};
  const float dist2 = edot(p, p);
  tOut = t;
  return (divisor != 0.f) & (tnear <= t) & (t <= 3.402823466e+38f) & (dist2 < radius * radius);
}
__device__ __forceinline__ bool local_disc_hit_uniform(const V3 &ro, const V3 &rd, const V3 &c, const V3 &n, float prod, float nro,
                                                       float thresh) {
  const float ddneg = vdot(c, n);
  const float tt = (ddneg - nro) / prod;
  V3 hp = V3{rd.x * tt + ro.x, rd.y * tt + ro.y, rd.z * tt + ro.z};
  hp.x = hp.x - c.x;
  hp.y = hp.y - c.y;
  hp.z = hp.z - c.z;
  return !(prod > 0.f) & !(fabsf(prod) < 1e-6f) & !(tt <= 0.f) & (vdot(hp, hp) < thresh);
}

} // namespace vr
