// vr_planar_lattice.hpp — the lattice table of a planar cloud whose centres sit on a square lattice, and the index window
// of a packet round in it (trace_kernel MODE_ABSORB_FLAT_LATTICE; pq_hit_lattice, vr_packet_query.hpp): the
// arithmetic, the host's rule for the table and the per-disk rule of the kernel that fills it.  Plain floats, no HIP type
// in here: tests/aux/planar_lattice.cpp compiles this file with the host compiler alone.
//
// Lattice cloud: planar disks (vr_planar_disks.hpp) in three dimensions whose centres, along the two in-plane axes b1 < b2,
// lie within delta / 8 of the points phase + k delta of a square lattice — delta the scene's gridDelta, phase the smallest
// centre coordinate per axis — no two of them at one lattice point, the lattice n1 x n2 points with n1 n2 <= 4 N.  The
// table is uint32[n2][n1]: the LEAF POSITION of the disk at lattice point (i, j), VR_LATTICE_EMPTY where there is none
// (holes are allowed).  Every initial surface of a level set is such a cloud.
//
// Why the window finds the parent's candidates.  The round's box [lo, hi] per in-plane axis is the parent's (pq_hit_packet
// ROUND: the box around the wave's plane hits, padded).  The parent's ball-box filter keeps a record with
// c - r <= hi and c + r >= lo (float sums), so a kept disk has lo - r (1 + 2^-22) <= c <= hi + r (1 + 2^-22) in real numbers
// (vr_planar_disks.hpp (2)).  Its lattice point x = phase + k delta is within delta / 8 of c, so
// lo - R <= x <= hi + R with R = r (1 + 2^-22) + delta / 8, and k lies in [(lo - R - phase) / delta, (hi + R - phase) / delta].
// lattice_axis_window takes the integers of that interval with R + pad in place of R: the pad (1e-5 of the largest
// coordinate) is three orders above the rounding of the two differences, of the product with fl(1 / delta) (relative
// 2^-23 of a coordinate difference) and of the kernel's own float test of the delta / 8 rule (lattice_cell_of).  Along the
// plane's axis every centre carries one word and the box is that word -+ pad: nothing to select.  So every record the
// parent's filter keeps belongs to a cell of the window; the kernel applies THE SAME filter to the records of the window's
// cells, on the same box and the same record bits: the candidate set is the parent's.  The candidates arrive in another
// order; the closest-hit rule (hit_update_lds: t, then the smaller original id) and the int64 flux sums do not depend on it.
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

constexpr uint32_t VR_LATTICE_EMPTY = 0xFFFFFFFFu;
constexpr int VR_LATTICE_MAX_AXIS = 1 << 20;  // lattice points per axis: far inside the floats' exact integers
constexpr int VR_LATTICE_WINDOW = 64;         // cells of a round's window: one per lane

// ---- the host's rule for the table --------------------------------------------------------------------------------
// The lattice's extent along one axis from the smallest and largest centre coordinate: round((hi - lo) / delta) + 1
// points, or 0 where there is no such lattice (no pitch, a non-finite extent, too many points).
inline int lattice_axis_points(float lo, float hi, float delta) {
  if (!(delta > 0.f) || !(hi >= lo))
    return 0;
  const float cells = (hi - lo) / delta;
  if (!(cells <= (float)(VR_LATTICE_MAX_AXIS - 1)))
    return 0;
  return (int)__builtin_rintf(cells) + 1;
}
// n1 x n2 points for N disks: a table of at most 4 N words (a cloud with holes, not a sparse one)
inline bool lattice_table_fits(int n1, int n2, uint32_t N) {
  return n1 >= 1 && n2 >= 1 && N >= 1u && N < (1u << 28) && (uint64_t)n1 * (uint64_t)n2 <= 4ull * N;
}
// the window's reach beyond the round's box (R + pad above)
inline float lattice_reach(float radius, float delta, float pad) { return radius * (1.f + 2.384185791015625e-07f) + pad + 0.125f * delta; }
// Can the window of a box one lattice cell wide hold its cells in VR_LATTICE_WINDOW lanes?  (A cloud of disks many cells
// wide: every round would fall back.)  The largest count of integers in an interval of length 2 reach / delta + 1, squared.
inline bool lattice_window_pays(float reach, float invDelta) {
  const float span = 2.f * reach * invDelta + 2.f;
  return span * span <= (float)VR_LATTICE_WINDOW;
}

// ---- per disk (the kernel that validates and fills the table) -----------------------------------------------------
// The lattice index of centre coordinate c along one axis; false where c is farther than delta / 8 from its lattice
// point, outside the n points, or not finite.
VR_HD bool lattice_cell_of(float c, float phase, float invDelta, int n, int &k) {
  const float f = (c - phase) * invDelta;
  const float r = __builtin_rintf(f);
  const bool ok = (__builtin_fabsf(f - r) <= 0.125f) & (r >= 0.f) & (r <= (float)(n - 1)); // (a NaN fails all three)
  k = ok ? (int)r : 0;
  return ok;
}

// ---- per round ----------------------------------------------------------------------------------------------------
// The lattice indices k0 .. k1 (inclusive; k0 > k1: none) along one axis whose points can lie within `reach` of
// [lo, hi], clamped to the table's 0 .. n - 1.  Both ends pass through a clamp in float before the conversion, so a box
// far outside the table — or a NaN — gives an empty or a clamped window, never an index outside the table.
VR_HD void lattice_axis_window(float lo, float hi, float phase, float invDelta, float reach, int n, int &k0, int &k1) {
  const float a = ((lo - reach) - phase) * invDelta, b = ((hi + reach) - phase) * invDelta;
  const float top = (float)(n - 1);
  const float ac = __builtin_fminf(__builtin_fmaxf(a, 0.f), top + 1.f); // (fmaxf / fminf of a NaN: the other operand)
  const float bc = __builtin_fmaxf(__builtin_fminf(b, top), -1.f);
  k0 = (int)__builtin_ceilf(ac);
  k1 = (int)__builtin_floorf(bc);
}
// Lane l's cell of a window w cells wide (1 <= w <= 64, 0 <= l < 64): column l % w, row l / w, without an integer
// division: (l + 1/2) / w is at least 1 / (2 w) >= 1 / 128 away from every integer, the reciprocal and the product are
// within a few 2^-24 of a value below 65.
VR_HD void lattice_lane_cell(int l, int w, float invW, int &col, int &row) {
  row = (int)(((float)l + 0.5f) * invW);
  col = l - row * w;
}

// ==== four corners per lane (trace_kernel MODE_ABSORB_FLAT_LATTICE_LANES; pq_hit_lattice_lanes, vr_packet_query.hpp) ==========
// A round's point q (vr_planar_disks.hpp (1)) lies in one lattice cell; where the disks are small enough against the pitch,
// only the lattice points at that cell's four corners can carry a disk that accepts q.  Each lane then tests its own four
// disks instead of every candidate of the wave's window.
//
// The rule, per in-plane axis, with u the point's coordinate, x = phase + k delta a lattice point (real numbers: phase and
// delta are floats), c the centre of the disk filed at x, r the radius, C a bound on |u| and |phase| and ulp the
// spacing of the floats at C:
//   acceptance: planar_round_cand accepts (either test: both thresholds are at most r^2 rounded, uniform_disk_threshold)
//     only where fl(u - c)^2 < r^2 in float, so |u - c| < r (1 + 2^-22) in real numbers (vr_planar_disks.hpp (2)).
//   the centre: lattice_cell_of filed c at x because |f - rint(f)| <= 1/8 for f = fl(fl(c - phase) invD), invD = fl(1 / delta).
//     f - rint(f) is exact; f itself differs from (c - phase) / delta by e / delta with
//       e <= |fl(c - phase) - (c - phase)| + |fl(c - phase)| (2^-24 + 2^-24 + 2^-48)   (the product's rounding, invD's)
//         <= ulp + 2 C 2.0001 2^-24 < ulp + 4.001 ulp                                     (|c - phase| <= 2 C; C 2^-24 < ulp)
//     so |c - x| <= delta / 8 + 5.001 ulp.
//   the cell: lattice_lane_corner takes i = floor(g), g = fl(fl(u - phase) invD): the same two roundings, |g delta -
//     (u - phase)| < 5.001 ulp.
// An accepting disk's lattice point has |u - x| < R = r (1 + 2^-22) + delta / 8 + 5.001 ulp, i.e. |(u - phase) / delta - k|
// < R / delta, and |g - k| < (R + 5.001 ulp) / delta.  Where
//       r (1 + 2^-22) + delta / 8 + 12 ulp <= delta                                        (lattice_lanes_rule)
// (12 ulp: the two 5.001 with room to spare) that is |g - k| < 1: k = floor(g) or floor(g) + 1, a corner of the cell.
// A point with |u| > C: C is the scene's largest coordinate plus two pitches (lattice_lanes_coord), every centre lies in the
// scene box and every lattice point within delta / 8 + 5.001 ulp of one, so such a point is farther than delta >= R from
// every lattice point and no disk accepts it, whichever cell the arithmetic names.  Testing a corner that does not accept is
// harmless: the test is planar_round_cand on the disk's own record.  Both ends of the index pass through a clamp in float
// before the conversion (as in lattice_axis_window): an infinite or NaN point names a cell outside the table, never an
// index a conversion made up.
constexpr float VR_LATTICE_LANES_ULPS = 12.f;
// the bound C on an in-plane coordinate that matters: the scene's largest (scene_scale, vr_prepare.cpp) and two pitches
inline float lattice_lanes_coord(float sceneScale, float delta) { return sceneScale + 2.f * delta; }
// the rule above, in double on the host (the three terms and delta are floats: their sum is exact enough by 2^-29)
inline bool lattice_lanes_rule(float radius, float delta, float C) {
  if (!(radius > 0.f) || !(delta > 0.f) || !(C >= 0.f) || !(C < 1e30f))
    return false;
  const double ulp = (double)__builtin_nextafterf(C, __builtin_inff()) - (double)C;
  return (double)radius * (1.0 + 2.384185791015625e-07) + 0.125 * (double)delta + (double)VR_LATTICE_LANES_ULPS * ulp <= (double)delta;
}
// The lower corner's lattice index along one axis, -1 .. n (n the axis's points): floor((u - phase) / delta), clamped in
// float first.  The cell's two corners along the axis are k and k + 1; each is a lattice point only where 0 <= . < n.
VR_HD int lattice_lane_corner(float u, float phase, float invDelta, int n) {
  const float g = (u - phase) * invDelta;
  const float gc = __builtin_fminf(__builtin_fmaxf(g, -1.f), (float)n); // (fmaxf / fminf of a NaN: the other operand)
  return (int)__builtin_floorf(gc);
}
// The window slot (the lane that owns the cell, lattice_lane_cell) of lattice point (i, j) in the window i0 .. i1 x
// j0 .. j1, or -1 where the point lies outside it.  The window lies inside the table and has at most VR_LATTICE_WINDOW
// cells, so a slot that is not -1 is below VR_LATTICE_WINDOW and names a cell of the table.
VR_HD int lattice_window_slot(int i, int j, int i0, int i1, int j0, int j1) {
  const bool in = (i >= i0) & (i <= i1) & (j >= j0) & (j <= j1);
  return in ? (j - j0) * (i1 - i0 + 1) + (i - i0) : -1;
}

} // namespace vr
