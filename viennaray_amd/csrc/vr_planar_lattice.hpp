// vr_planar_lattice.hpp — the lattice table of a planar cloud whose centres sit on a square lattice, and the index window
// of a packet round in it (trace_kernel_lattice, vr_trace.hip; pq_hit_lattice, vr_packet_query.hpp): the
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

} // namespace vr
