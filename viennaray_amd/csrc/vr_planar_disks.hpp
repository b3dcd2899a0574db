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

// ==== one point per round (trace_kernel MODE_ABSORB_FLAT_PLANAR_ROUND; pq_hit_packet ROUND) ===============================
// Three further things that are the ray's own on a planar cloud: the two tests share one point, the query's box follows
// from that point, and a ray that starts and lands well inside the wall rectangle needs no wall test.
//
// (1) One point for both tests.  With n = +-e_a exactly (s = n[a], the two other components zeros of either sign) and
// finite operands:
//   divisor = edot(d, n) = d.x n.x + (d.y n.y + d.z n.z) and prod = vdot(n, d) = (n.x d.x + n.y d.y) + n.z d.z: the two
//   products with a zero are +-0, the third is d[a] * s exactly; both sums are d[a] * s where that is not a zero, and
//   zeros (of signs that may differ) where it is.  A zero divisor fails the hit test's divisor != 0, a zero prod the
//   neighbour test's |prod| >= 1e-6: with da = d[a] * s in place of both, every condition on divisor or prod has the value
//   it had, and a division by it gives the same bits wherever either test can still accept.
//   numerators: (ca - oa) * s is +-fl(ca - oa) (s = +-1: exact).  ca * s - nro with nro = vdot(n, o) = o[a] * s (or a
//   zero where o[a] is one): +-ca -+ o[a] rounds to +-fl(ca - oa), round-to-nearest being symmetric; with o[a] = +-0 both
//   are ca * s, unless ca is a zero too.  So the numerators are equal or both zeros; a zero numerator gives t = tt = +-0
//   (or NaN): tnear <= t fails, and tt <= 0 holds or the NaN fails the distance comparison below.
//   points: q = o + d t and g = d tt + o are the same product and the same sum in each coordinate (both commute).
// Hence t == tt and q == g bit for bit wherever either test can accept, and where they might differ both tests reject.
// The round keeps t, q and the two acceptance conditions; each condition is folded into ITS threshold — radius^2 /
// thresh where it holds, 0 where it fails or the lane takes no part: no squared distance (>= 0, or a NaN) is below 0 —
// so q carries no NaN of the folding's making and can feed the box (2) and the wall rule (3).  A non-finite t or q
// (origin or direction out of range) makes the squared distance an infinity or a NaN: both comparisons fail, as they do
// in planar_hit_cand / planar_local_cand.  Per candidate: q - c once, each difference squared once, and the two sums in
// their own associations (edot: x + (y + z); vdot: (x + y) + z) against the two thresholds.
struct PlanarRound {
  float t, qx, qy, qz;
  float hitThr, locThr; // radius^2 / thresh where the hit / neighbour test's conditions on the ray hold, else 0
};
// oa = o[a], da = d[a] * s; on: the lane takes part
VR_HD PlanarRound planar_round_point(bool on, float ox, float oy, float oz, float dx, float dy, float dz, float oa, float da, float tnear,
                                     float ca, float s, float radius, float thresh) {
  PlanarRound r;
  r.t = ((ca - oa) * s) / da;
  const bool okH = on & (da != 0.f) & (tnear <= r.t) & (r.t <= 3.402823466e+38f);
  const bool okL = on & !(da > 0.f) & !(__builtin_fabsf(da) < 1e-6f) & !(r.t <= 0.f);
  r.qx = ox + dx * r.t;
  r.qy = oy + dy * r.t;
  r.qz = oz + dz * r.t;
  r.hitThr = okH ? radius * radius : 0.f;
  r.locThr = okL ? thresh : 0.f;
  return r;
}
VR_HD void planar_round_cand(const PlanarRound &r, float cx, float cy, float cz, bool &hit, bool &local) {
  const float px = r.qx - cx, py = r.qy - cy, pz = r.qz - cz;
  const float xx = px * px, yy = py * py, zz = pz * pz;
  hit = xx + (yy + zz) < r.hitThr;   // (edot)
  local = (xx + yy) + zz < r.locThr; // (vdot)
}

// (2) The query's box from q.  A ray meets the cloud's plane in q alone, so the box around the q of the lanes that can
// hit (hitThr > 0; crediting needs a geometry hit) serves in place of the box around the rays' stretches through the
// scene box: a disk accepted by either test has its centre within radius (1 + 2^-22) of q per coordinate — the squared
// differences are not negative, so each is below the threshold — and the rounding of the differences, of the ball filter's
// c -+ r and of the boxes is a few ulp of the largest coordinate, which the pad (1e-5 of it) covers.  So the disk passes
// the ball-box filter and its leaf node's box meets the box; the closest-hit rule makes the result independent of which
// further candidates were found.  Along a the box is the constant interval ca -+ pad (planar_round_box below).  A lane
// whose q lies outside the scene box (by more than the pad) hits nothing and stays out, which also keeps infinities and
// NaNs out of the reductions.
// b1 < b2: the two in-plane axes of a
VR_HD void planar_in_plane_axes(int a, int &b1, int &b2) {
  b1 = a == 0 ? 1 : 0;
  b2 = a == 2 ? 1 : 2;
}
// does the lane's q count for the box?  u, v = q[b1], q[b2]; sb = {lo1 - pad, hi1 + pad, lo2 - pad, hi2 + pad} of the scene
// box along b1, b2; tWall: the lane's wall hit (infinite: none) — a wall met before the plane wins whatever the disks do
VR_HD bool planar_round_valid(const PlanarRound &r, float u, float v, float tWall, float sLo1, float sHi1, float sLo2, float sHi2) {
  return (r.hitThr > 0.f) & !(tWall < r.t * 0.99999f) & (sLo1 <= u) & (u <= sHi1) & (sLo2 <= v) & (v <= sHi2);
}

// (3) Wall-free rays.  The walls are the four sides of the rectangle [lo, hi] x [lo, hi] along the two wall axes
// (hit_walls_from, vr_intersect.hpp).  A lane is wall-free when, per wall axis, lo <= o <= hi and lo + m <= q <= hi - m
// with m = 0.002 (hi - lo).  For such a lane with t > 0, and per axis (e = hi - lo, C = max(|lo|, |hi|)):
//   only the wall the ray moves towards passes wall_reachable; take W = hi, d > 0 (W = lo mirrors it).
//   In real numbers d t = q' - o with |q' - q| <= 2 ulp(C) <= 2.4e-7 C (one product, one sum); o >= lo and q <= hi - m
//   give d t <= e, and the wall plane's parameter tw' = (hi - o) / d >= t + (m - 2.4e-7 C) / d >= t (1 + (m - 2.4e-7 C) / e).
//   The host hands out the shrunk rectangle only where C <= 1000 e (else an empty one: no lane is wall-free), so
//   tw' >= t (1 + 0.002 - 2.4e-4) = 1.00176 t.
//   The pre-test's tw = fl(fl(W - o) * rcp(d)) is within 3e-7 relative of tw' (one difference, one reciprocal of 1 ulp,
//   one product), its limit fl(h.t * 1.001f) within 6e-8 of 1.001 t where h.t = t: tw >= 1.00175 t > limit, and the wall is
//   rejected in float before any triangle test.  (An overflowing rcp gives tw = inf: rejected too.)
// So for a wall-free lane whose closest hit is the plane's (h.t = t) the wall test changes nothing, and an exact wall
// hit lies at about tw', never before t: tWall cannot exclude it from the box.  A wall-free lane without a geometry hit
// (a hole in the cloud, t <= 0, a ray along the plane) gets the full wall test.
struct PlanarWallRect {
  float lo1, hi1, lo2, hi2;
};
// the host's rule for one wall axis: the shrunk interval, or an empty one where the argument above does not hold
inline void planar_wall_inner(float lo, float hi, float &inLo, float &inHi) {
  const float e = hi - lo, C = __builtin_fabsf(lo) > __builtin_fabsf(hi) ? __builtin_fabsf(lo) : __builtin_fabsf(hi);
  const float m = 0.002f * e;
  inLo = lo + m;
  inHi = hi - m;
  if (!(e > 0.f) || !(C <= 1000.f * e) || !(inLo <= inHi)) { // (also a NaN or an infinite extent)
    inLo = __builtin_inff();
    inHi = -__builtin_inff();
  }
}
// o1, o2, q1, q2: the origin and q along the two wall axes; w: the walls' rectangle, in: the shrunk one
VR_HD bool planar_wall_free(float o1, float o2, float q1, float q2, const PlanarWallRect &w, const PlanarWallRect &in) {
  return (w.lo1 <= o1) & (o1 <= w.hi1) & (w.lo2 <= o2) & (o2 <= w.hi2) & (in.lo1 <= q1) & (q1 <= in.hi1) & (in.lo2 <= q2) &
         (q2 <= in.hi2);
}

} // namespace vr
