// vr_planar_disks.hpp — the candidate tests of the packet query for PLANAR uniform disks (pq_hit_packet PLANAR,
// vr_packet_query.hpp): the arithmetic, and the host's rule for the shared normal.  Plain floats, no HIP type in here:
// tests/aux/planar_disks.cpp compiles this file with the host compiler alone.
//
// Planar disks: uniform disks (one normal n, one radius: vr_context::uniformDisks) whose normal has one component of
// exactly +-1 (axis a, s = n[a]) and two components that are zeros of either sign, whose centres all carry the same
// 32-bit word ca in coordinate a, and whose centre coordinates are all finite.  The initial surface of a process
// simulation is such a cloud.  Where a ray crosses the disks' common plane is then a property of the ray, not of the
// candidate, and so is everything hit_disc_uniform / local_disc_hit_uniform (vr_intersect.hpp) compute before they
// subtract the centre:
//
// Hit test.  edot(c - o, n) = co.x n.x + (co.y n.y + co.z n.z): the two products with a zero are +-0 (finite operands),
// the product with +-1 is exact, so the sum is (ca - o[a]) * s — the operations below — whenever that is non-zero, and
// otherwise a zero whose sign depends on the candidate.  A zero numerator gives t = +-0, or a NaN over a zero divisor:
// tnear <= t fails either way (tnear is 1e-4, never below), and t is read only where the test passed.  Hence t, the
// point q = o + d t and the three range conditions are the ray's; per candidate (q - c) — the existing form is
// (o.x + d.x t) - c.x, the same association — and edot(p, p) < radius^2 remain.
//
// Neighbour test.  ddneg = (c.x n.x + c.y n.y) + c.z n.z is ca * s exactly, or a zero of candidate-dependent sign where
// ca is a zero; ddneg - nro is then -nro exactly unless nro is a zero too, and in that case tt = +-0 (or a NaN over a
// zero prod, which |prod| < 1e-6 rejects): tt <= 0 rejects it whatever the sign.  Hence tt, g = rd tt + ro and the three
// sign conditions are the ray's; per candidate hp = g - c and vdot(hp, hp) < thresh remain.
//
// A ray origin with a non-finite component is rejected by both forms: the existing ones through a NaN numerator
// (inf x 0, or inf - inf), these through an infinite or NaN squared distance (q and g inherit the component).
//
// The conditions that are the ray's are folded into the point: where one fails — or the lane takes no part — the
// point's first coordinate is a NaN, the squared distance with it, and the candidate's comparison fails.  That keeps
// the round's terms in vector registers alone (the flat-scene kernel has no scalar register to spare for two masks).
#pragma once
#include <cstdint>

#ifndef VR_HD
#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define VR_HD __host__ __device__ __forceinline__
#else
#define VR_HD inline
#endif
#endif

namespace vr {

// ---- the host's rule for the shared normal -----------------------------------------------------------------------
// The axis a of a planar cloud from the three words of its normal: one word is +-1.0f, the two others are +-0.
// -1: no such axis (0.99999994, a denormal beside the 1, a NaN: all refused).
inline int planar_disk_axis(const uint32_t (&n)[3]) {
  int axis = -1;
  for (int k = 0; k < 3; ++k) {
    const uint32_t w = n[k] & 0x7FFFFFFFu;
    if (w == 0x3F800000u && axis < 0)
      axis = k;
    else if (w != 0u)
      return -1;
  }
  return axis;
}

// ---- per ray and round --------------------------------------------------------------------------------------------
// the hit test's terms: t, and q = o + d t (q.x a NaN where the ray can hit no candidate)
struct PlanarHit {
  float t, qx, qy, qz;
};
// oa = o[a]; divisor = edot(d, n), the caller's as in hit_disc_uniform; on: the lane takes part
VR_HD PlanarHit planar_hit_round(bool on, float ox, float oy, float oz, float dx, float dy, float dz, float oa, float tnear, float ca,
                                 float s, float divisor) {
  PlanarHit r;
  r.t = ((ca - oa) * s) / divisor;
  const bool ok = on & (divisor != 0.f) & (tnear <= r.t) & (r.t <= 3.402823466e+38f);
  const float qx = ox + dx * r.t;
  r.qx = ok ? qx : __builtin_nanf("");
  r.qy = oy + dy * r.t;
  r.qz = oz + dz * r.t;
  return r;
}
// the neighbour test's terms: g = rd tt + ro (g.x a NaN where the ray credits no candidate)
struct PlanarLocal {
  float gx, gy, gz;
};
// prod = vdot(n, rd), nro = vdot(n, ro): the caller's as in local_disc_hit_uniform
VR_HD PlanarLocal planar_local_round(bool on, float rox, float roy, float roz, float rdx, float rdy, float rdz, float ca, float s,
                                     float prod, float nro) {
  PlanarLocal r;
  const float tt = (ca * s - nro) / prod;
  const bool ok = on & !(prod > 0.f) & !(__builtin_fabsf(prod) < 1e-6f) & !(tt <= 0.f);
  const float gx = rdx * tt + rox;
  r.gx = ok ? gx : __builtin_nanf("");
  r.gy = rdy * tt + roy;
  r.gz = rdz * tt + roz;
  return r;
}

// ---- per candidate (centre c) -------------------------------------------------------------------------------------
VR_HD bool planar_hit_cand(const PlanarHit &r, float cx, float cy, float cz, float radius) {
  const float px = r.qx - cx, py = r.qy - cy, pz = r.qz - cz;
  const float dist2 = px * px + (py * py + pz * pz); // (edot)
  return dist2 < radius * radius;
}
VR_HD bool planar_local_cand(const PlanarLocal &r, float cx, float cy, float cz, float thresh) {
  const float hx = r.gx - cx, hy = r.gy - cy, hz = r.gz - cz;
  return (hx * hx + hy * hy) + hz * hz < thresh; // (vdot)
}

} // namespace vr
