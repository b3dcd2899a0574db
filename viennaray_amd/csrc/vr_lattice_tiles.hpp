// vr_lattice_tiles.hpp — the tiles of a lattice table (vr_planar_lattice.hpp) that the tile-bucket pipeline files its
// rays by (gen_tile_kernel, tile_trace_kernel: vr_tile_buckets.hpp): the index arithmetic and the host's sizing rules.
// Plain C++, no HIP type in here: tests/aux/lattice_tiles.cpp compiles this file with the host compiler alone.
//
// A point's cell along one axis is k = lattice_lane_corner(u) in -1 .. n (n the axis's lattice points); the disks that can
// accept the point sit at lattice indices k and k + 1 (the four-corner rule).  With T = 2^shift cells per tile and axis,
// cell k belongs to tile t = (k + 1) >> shift: tile t holds the cells t T - 1 .. t T + T - 2, whose corners are the
// lattice indices t T - 1 .. t T + T - 1 — T + 1 points per axis, the tile's own T and a halo of one, some of them outside
// the table (index -1, or >= n) on a border tile.  Cells -1 .. n need ((n + 1) >> shift) + 1 tiles per axis.
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

constexpr int VR_TILE_SHIFT_MIN = 1, VR_TILE_SHIFT_MAX = 6; // 2 .. 64 cells per tile and axis
constexpr uint32_t VR_TILE_MAX_TILES = 1024u;               // tiles of a launch: a counter each in the generator's LDS

// the tile of cell k (-1 .. n) along one axis
VR_HD int lattice_tile_of(int k, int shift) { return (k + 1) >> shift; }
// tiles along an axis of n lattice points
inline int lattice_tiles_axis(int n, int shift) { return ((n + 1) >> shift) + 1; }
// the first lattice index of tile t's points (-1 for tile 0), and the points per axis
VR_HD int lattice_tile_first(int t, int shift) { return (t << shift) - 1; }
VR_HD int lattice_tile_width(int shift) { return (1 << shift) + 1; }
// The slot of lattice index (i, j) among the (T + 1)^2 points of tile (ti, tj), row-major, or -1 where the index lies
// outside the tile and its halo: a slot that is not -1 is below lattice_tile_width^2.
VR_HD int lattice_tile_slot(int i, int j, int ti, int tj, int shift) {
  const int W = lattice_tile_width(shift);
  const int li = i - lattice_tile_first(ti, shift), lj = j - lattice_tile_first(tj, shift);
  const bool in = (li >= 0) & (li < W) & (lj >= 0) & (lj < W);
  return in ? lj * W + li : -1;
}

// ---- the host's sizing rules ----------------------------------------------------------------------------------------
// LDS bytes of a tile in tile_trace_kernel: per point {leaf position, centre} (16), the original id (4), a counter (4)
inline uint32_t lattice_tile_lds_bytes(int shift) {
  const uint32_t W = (uint32_t)lattice_tile_width(shift);
  return W * W * 24u;
}
// Record slots of one tile's bucket for a batch of `rays` rays from a source rectangle of area srcArea, the tile
// tileSide x tileSide: a ray's landing point is its origin — uniform over the rectangle — plus an offset that does not
// depend on it, so the landing density nowhere exceeds rays / srcArea.  The expected count under that bound, eight
// standard deviations of a Poisson count and a constant for the smallest batches; what does not fit goes to the overflow region.
inline uint32_t lattice_tile_capacity(uint64_t rays, double tileSide, double srcArea) {
  double share = srcArea > 0. ? tileSide * tileSide / srcArea : 1.;
  if (!(share < 1.))
    share = 1.;
  const double mean = (double)rays * share;
  double cap = mean + 8. * __builtin_sqrt(mean) + 64.;
  if (cap > (double)rays)
    cap = (double)rays;
  return (uint32_t)cap + 1u;
}

} // namespace vr
