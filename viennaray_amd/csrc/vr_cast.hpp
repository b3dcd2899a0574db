// vr_cast.hpp — the per-ray bookkeeping of castRays (vr_cast.hip: cast_rays_kernel), in plain C++: the host compiler takes
// this file alone (tests/aux/cast_rays.cpp), the kernel includes it.  A ray is a chain of segments; every finished segment
// — the closest hit of one walk plus the wall test — is folded into the ray's state here, and the state becomes the four
// outputs at the end.  include/viennaray_amd.h has the definition this implements.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define VR_CAST_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define VR_CAST_FN inline
#endif

namespace vr {

constexpr int32_t CAST_MISS = -1; // VR_CAST_MISS: left the scene, passed an IGNORE wall, or beyond tmax
constexpr int32_t CAST_WALL = -2; // VR_CAST_WALL: stopped on a wall (following off, or the boundary-hit budget ran out)

struct CastState {
  float dist;            // float32 sum of the segments' t, added in segment order
  uint32_t boundaryHits; // walls the ray was continued at: reflected, wrapped, or passed from the back side
  int32_t prim;          // the result code once the ray has ended
};

enum CastNext {
  CAST_END = 0,   // the ray has ended: s.prim holds its code
  CAST_AT_WALL = 1 // a wall the ray is followed at: the caller applies the wall's rule (process_boundary_hit), then either
                   // traces on from the new origin or, where the wall is IGNORE, calls cast_ignored
};

VR_CAST_FN void cast_begin(CastState &s) {
  s.dist = 0.f;
  s.boundaryHits = 0u;
  s.prim = CAST_MISS;
}

// One finished segment: geom -1 miss / 0 wall / 1 geometry (HitRec::geom), prim the wall or original primitive id, t the
// segment's parameter.  dist only ever grows (t >= tnear >= 0), so a ray whose length has passed tmax can end at once: run
// to its end it could only end further out, and beyond tmax every outcome is a miss.  A hit at exactly tmax counts.
// The budget is the tracer's comparison (++boundaryHits > maxBoundaryHits); the count kept is of the walls passed, so it
// stays at maxBoundaryHits on the wall that exceeds it.
VR_CAST_FN CastNext cast_segment(CastState &s, int geom, uint32_t prim, float t, bool follow, uint32_t maxBoundaryHits,
                                 float tmax) {
  if (geom < 0) {
    s.prim = CAST_MISS;
    return CAST_END;
  }
  s.dist = s.dist + t;
  if (s.dist > tmax) {
    s.prim = CAST_MISS;
    return CAST_END;
  }
  if (geom == 1) {
    s.prim = (int32_t)prim;
    return CAST_END;
  }
  const uint32_t hits = s.boundaryHits + 1u;
  if (!follow || hits > maxBoundaryHits || hits == 0u) { // (hits == 0: the counter would wrap; never with a real budget)
    s.prim = CAST_WALL;
    return CAST_END;
  }
  s.boundaryHits = hits;
  return CAST_AT_WALL;
}

// the wall of the last cast_segment was IGNORE: the ray leaves the scene through it
VR_CAST_FN void cast_ignored(CastState &s) {
  s.boundaryHits -= 1u;
  s.prim = CAST_MISS;
}

// The outputs of an ended ray.  A miss has distance +inf.  With a finite tmax a miss also reports no boundary hits: such
// a ray may have been stopped early, and "unbounded, then everything beyond tmax turned into a miss" must not depend on
// where (an unbounded cast keeps the count of a ray that left the scene).  `hit` says whether the last segment's point
// org + dir * t is an output (false: NaN).
VR_CAST_FN void cast_finish(const CastState &s, float tmax, int32_t &prim, float &dist, uint32_t &boundaryHits, bool &hit) {
  const float inf = __builtin_huge_valf();
  const bool miss = s.prim == CAST_MISS;
  prim = s.prim;
  dist = miss ? inf : s.dist;
  boundaryHits = (miss && tmax < inf) ? 0u : s.boundaryHits;
  hit = !miss;
}

} // namespace vr
