// vr_bin_grid.hpp — the sort-bin grid of the ray generator: how the far-plane cells are sized (host) and how a folded
// position maps to its cell and bin (host and device).  No HIP type in here: tests/aux/bin_grid.cpp compiles this file
// with the host compiler alone.
//
// Two grids.  The PLAIN grid cuts the domain into ceil(sqrt(rays / raysPerBin)) equal cells per axis, wherever their edges
// fall.  The ALIGNED grid (3-D, disks, gridDelta > 0) knows that the disks of a flat stretch of surface sit on a lattice
// of pitch gridDelta: per in-plane axis its origin lies on a lattice line through a disk centre, at or below the
// domain's lower end, and its cell is m lattice cells or 1 / k of one.  A trace round's 64 rays span two or three
// consecutive bins of a tile column; where that column is exactly one lattice cell wide, with its edges on the lines
// through the centres, the round's box (widened by 2 r) meets two lattice columns, not three or four.
#pragma once
#include <algorithm>
#include <cmath>
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

constexpr int32_t VR_BIN_AXIS_MAX = 4096; // cells per axis of a 3-D grid

// ---- the key (host and device) ---------------------------------------------------------------------------------
// a coordinate in units of the domain's extent, folded back into [0, 1] the way the side walls would
VR_HD float fold_unit(float u, int bc) {
  if (bc == 1) // periodic
    return u - floorf(u);
  if (bc == 0) { // reflective: mirror fold with period 2
    float v = u - 2.f * floorf(0.5f * u);
    return v > 1.f ? 2.f - v : v;
  }
  return u; // ignore: clamped in bin_cell
}

// cell of the folded position u along one axis: (u x ext + (lo - origin)) x invCell in ONE fused multiply-add, with
// scale = ext x invCell and bias = (lo - origin) x invCell made on the host in double (the plain grid: scale = T, bias = 0)
VR_HD int bin_cell(float u, float scale, float bias, int T) {
  const int c = (int)__builtin_fmaf(u, scale, bias);
  return c < 0 ? 0 : (c >= T ? T - 1 : c);
}

// 8x8 tiles in row-major order; inside a tile the COLUMNS (constant c1) run in alternating directions (boustrophedon:
// up column 0, down column 1, ...), so consecutive bins are always adjacent cells — also from one tile to the next in a
// row of tiles (a tile ends bottom right, its neighbour starts bottom left).  A round of the trace kernel swallows two
// or three bins; with plain row-major cells one round in four straddled a row end: a packet box eight cells wide.
VR_HD unsigned bin_index(int c1, int c2, int tilesPerRow) {
  const unsigned tile = (unsigned)(c2 >> 3) * (unsigned)tilesPerRow + (unsigned)(c1 >> 3);
  const unsigned row = (unsigned)c2 & 7u, col = (unsigned)c1 & 7u;
  return tile * 64u + (col << 3 | ((col & 1u) ? 7u - row : row));
}

// ---- the grid (host) ----------------------------------------------------------------------------------------------
struct BinGrid {
  int32_t T1 = 1, T2 = 1;  // cells per axis
  int32_t tiles = 1;       // 8x8-cell tiles per row (3-D)
  uint32_t numBins = 1;
  float scale1 = 1.f, bias1 = 0.f, scale2 = 1.f, bias2 = 0.f; // bin_cell's
  // what the aligned rule chose (diagnostics and tests; the plain grid leaves them as they are)
  int32_t aligned = 0;
  int32_t m1 = 1, m2 = 1, k2 = 1;      // cell along axis 1: m1 lattice cells; along axis 2: m2 cells, or 1 / k2 of one
  double origin1 = 0., origin2 = 0.;   // first edge of either axis
  double cell1 = 0., cell2 = 0.;       // cell sizes
  double meanRays = 0.;                // mean rays per (whole) bin
};

// what the aligned rule is given
struct BinGridIn {
  uint64_t rays = 0;           // rays of the batch
  uint32_t perBin = 40;        // VR_RAYS_PER_BIN
  uint32_t binCap = 128;       // record slots per bin
  uint32_t ovCap = 0;          // record slots of the overflow region behind the bins
  float lo1 = 0, hi1 = 0, lo2 = 0, hi2 = 0; // the source plane's extent along firstDir / secondDir
  float phase1 = 0, phase2 = 0; // coordinates of one disk centre (the lattice's phase)
  float pitch = 0;             // gridDelta
};

// the plain grid: far-plane cells holding ~perBin rays each
inline BinGrid bin_grid_plain(int D, uint64_t rays, uint32_t perBin) {
  BinGrid g;
  const uint64_t target = rays / (perBin > 1u ? perBin : 1u) > 1 ? rays / (perBin > 1u ? perBin : 1u) : 1;
  if (D == 2) {
    g.T1 = (int32_t)(target < (1u << 22) ? target : (1u << 22));
    g.T2 = 1;
    g.tiles = 1;
    g.numBins = (uint32_t)g.T1;
  } else {
    double t = std::ceil(std::sqrt((double)target));
    t = t < 1.0 ? 1.0 : (t > (double)VR_BIN_AXIS_MAX ? (double)VR_BIN_AXIS_MAX : t);
    g.T1 = g.T2 = (int32_t)t;
    g.tiles = (g.T1 + 7) / 8;
    g.numBins = (uint32_t)g.tiles * (uint32_t)g.tiles * 64u;
  }
  g.scale1 = (float)g.T1;
  g.scale2 = (float)g.T2;
  g.meanRays = (double)rays / ((double)g.T1 * (double)g.T2);
  return g;
}

// bounds of the aligned grid's mean rays per bin: [want / 2, binCap / 2] with want = min(perBin, binCap / 2)
inline double bin_grid_mean_hi(const BinGridIn &in) { return 0.5 * (double)in.binCap; }
inline double bin_grid_mean_lo(const BinGridIn &in) {
  const double hi = bin_grid_mean_hi(in);
  return 0.5 * ((double)in.perBin < hi ? (double)in.perBin : hi);
}

// The aligned grid (3-D).  false: the rule's conditions cannot all be met — the caller keeps the plain grid.
//   rho = rays per lattice cell, want = min(perBin, binCap / 2);
//   dense (rho >= want): axis 1 (c1: consecutive bins of a tile column do not advance along it) gets ONE lattice cell,
//     axis 2 is cut into 1 / k2 of a cell, k2 = max(floor(rho / perBin), ceil(rho / (binCap / 2))): the mean rays per bin
//     stay in [perBin, 2 perBin) and never above half of binCap — bins FULLER than the plain grid's rather than emptier:
//     a finer second axis makes a tile column turn more often and was the loser in the model (tools/bin_order_sim.py);
//   sparse (rho < want): a bin covers A = want / rho whole lattice cells, m2 = floor(sqrt(A)) along axis 2 and
//     m1 = round(A / m2) along axis 1 (the model: 3 x 1 ahead of 1 x 3 and 2 x 2 at 12.5 rays per cell, 6 x 5 of 5 x 6 at 1.25);
//   at most VR_BIN_AXIS_MAX cells per axis, and numBins x binCap + ovCap fits the 32-bit slot index.
inline bool bin_grid_aligned(const BinGridIn &in, BinGrid &g) {
  const double d = (double)in.pitch;
  const double e1 = (double)in.hi1 - (double)in.lo1, e2 = (double)in.hi2 - (double)in.lo2;
  if (!(d > 0.) || !(e1 > 0.) || !(e2 > 0.) || in.rays == 0 || in.binCap < 2u || in.perBin < 1u)
    return false;
  if (!(e1 / d < 1e6) || !(e2 / d < 1e6)) // (the lattice arithmetic below stays exact to a small fraction of a cell)
    return false;
  const double rho = (double)in.rays * d * d / (e1 * e2); // rays per lattice cell
  const double meanHi = bin_grid_mean_hi(in), meanLo = bin_grid_mean_lo(in), want = 2. * meanLo;
  // origin: the lattice line at or below lo (1e-4 of a cell above it at most: float rounding of lo itself)
  const double o1 = (double)in.phase1 + std::floor(((double)in.lo1 - (double)in.phase1) / d + 1e-4) * d;
  const double o2 = (double)in.phase2 + std::floor(((double)in.lo2 - (double)in.phase2) / d + 1e-4) * d;
  const double span1 = ((double)in.hi1 - o1) / d, span2 = ((double)in.hi2 - o2) / d; // lattice cells to cover
  const double m1min = std::max(1., std::ceil(span1 / (double)VR_BIN_AXIS_MAX - 1e-9));
  const double m2min = std::max(1., std::ceil(span2 / (double)VR_BIN_AXIS_MAX - 1e-9));
  double m1 = m1min, m2 = 1., k2 = 1.;
  if (rho * m1 >= want) { // dense: one lattice cell along axis 1, 1 / k2 of one along axis 2
    const double rho1 = rho * m1;
    k2 = std::max(1., std::max(std::floor(rho1 / (double)in.perBin), std::ceil(rho1 / meanHi)));
    const double kmax = std::floor((double)VR_BIN_AXIS_MAX / span2);
    if (kmax < 1.) {
      k2 = 1.;
      m2 = m2min;
    } else if (k2 > kmax) {
      k2 = kmax;
    }
  } else { // sparse: a bin of A = want / rho lattice cells, m2 = floor(sqrt(A)) of them along axis 2, the rest along axis 1
    const double A = want / rho;
    m2 = std::max(m2min, std::floor(std::sqrt(A)));
    m1 = std::max(m1min, std::floor(A / m2 + 0.5));
    if (rho * m1 * m2 > meanHi && m1 > m1min)
      m1 -= 1.;
  }
  const double rho1 = rho * m1;
  if (!(m1 < 1e6) || !(m2 < 1e6) || !(k2 < 1e6))
    return false;
  const double mean = rho1 * m2 / k2;
  if (!(mean >= meanLo) || !(mean <= meanHi))
    return false;
  const double c1 = d * m1, c2 = d * m2 / k2;
  const double t1 = std::ceil(((double)in.hi1 - o1) / c1 - 1e-6), t2 = std::ceil(((double)in.hi2 - o2) / c2 - 1e-6);
  if (!(t1 <= (double)VR_BIN_AXIS_MAX) || !(t2 <= (double)VR_BIN_AXIS_MAX))
    return false;
  BinGrid r;
  r.T1 = t1 < 1. ? 1 : (int32_t)t1;
  r.T2 = t2 < 1. ? 1 : (int32_t)t2;
  r.tiles = (r.T1 + 7) / 8;
  const uint64_t nb = (uint64_t)r.tiles * (uint64_t)((r.T2 + 7) / 8) * 64u;
  if (nb * (uint64_t)in.binCap + (uint64_t)in.ovCap > 0xFFFFFFFFull)
    return false;
  r.numBins = (uint32_t)nb;
  r.scale1 = (float)(e1 / c1);
  r.bias1 = (float)(((double)in.lo1 - o1) / c1);
  r.scale2 = (float)(e2 / c2);
  r.bias2 = (float)(((double)in.lo2 - o2) / c2);
  r.aligned = 1;
  r.m1 = (int32_t)m1;
  r.m2 = (int32_t)m2;
  r.k2 = (int32_t)k2;
  r.origin1 = o1;
  r.origin2 = o2;
  r.cell1 = c1;
  r.cell2 = c2;
  r.meanRays = mean;
  g = r;
  return true;
}

} // namespace vr
