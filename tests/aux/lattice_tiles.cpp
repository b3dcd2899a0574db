// The tiles of a lattice table (vr_lattice_tiles.hpp) on the host, against brute force.  For lattices of 1, 2, 33 and 1000
// points per axis and every tile size 2 .. 64:
// (1) every cell -1 .. n has one tile, tiles are runs of T cells, the first starts at cell -1, and lattice_tiles_axis is the
//     number of distinct tiles;
// (2) a tile's points are the lattice indices first .. first + T: the corners of its cells, found by enumerating the cells;
//     lattice_tile_slot is the row-major index among them and -1 for every other index (two rings around the tile tried);
// (3) a point's four corners always lie in its tile + halo: random points and points on and next to the table's border,
//     also far outside it, infinite and NaN, go through lattice_lane_corner, and each corner has a slot below (T + 1)^2 in
//     the tile the cell names;
// (4) the sizing rules: the LDS of the largest tile fits a workgroup's, a bucket's capacity never falls with the rays and
//     holds the expected count.
// Plain C++17, vr_lattice_tiles.hpp and vr_planar_lattice.hpp alone.  tests/test_tile_buckets.py reads the last line.
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <set>

#include "vr_lattice_tiles.hpp"
#include "vr_planar_lattice.hpp"

using namespace vr;

static long failed = 0;
#define CHECK(cond)                                                                                                    \
  do {                                                                                                                 \
    if (!(cond)) {                                                                                                     \
      if (++failed <= 20)                                                                                              \
        std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);                                                 \
    }                                                                                                                  \
  } while (0)

static void check_axis(int n, int shift) {
  const int T = 1 << shift, W = lattice_tile_width(shift);
  CHECK(W == T + 1);
  std::set<int> tiles;
  for (int k = -1; k <= n; ++k) {
    const int t = lattice_tile_of(k, shift);
    tiles.insert(t);
    CHECK(t >= 0 && t < lattice_tiles_axis(n, shift));
    CHECK(t == (k + 1) / T);                                    // runs of T cells from cell -1 on
    const int first = lattice_tile_first(t, shift);
    CHECK(first == t * T - 1);
    CHECK(k >= first && k + 1 <= first + T);                     // both corners of the cell among the tile's points
    if (k > -1)
      CHECK(lattice_tile_of(k - 1, shift) == t || lattice_tile_of(k - 1, shift) == t - 1);
  }
  CHECK((int)tiles.size() == lattice_tiles_axis(n, shift));
  CHECK(*tiles.begin() == 0 && *tiles.rbegin() == lattice_tiles_axis(n, shift) - 1);
}

static void check_slots(int n1, int n2, int shift) {
  const int W = lattice_tile_width(shift);
  const int t1 = lattice_tiles_axis(n1, shift), t2 = lattice_tiles_axis(n2, shift);
  // (a big lattice: its corner tiles, a middle one and a few random ones)
  std::mt19937 rng(1234u + (unsigned)(n1 * 131 + n2 * 7 + shift));
  for (int pick = 0; pick < 12; ++pick) {
    int ti = pick == 0 ? 0 : pick == 1 ? t1 - 1 : pick == 2 ? t1 / 2 : (int)(rng() % (unsigned)t1);
    int tj = pick == 0 ? 0 : pick == 1 ? t2 - 1 : pick == 2 ? t2 / 2 : (int)(rng() % (unsigned)t2);
    const int i0 = lattice_tile_first(ti, shift), j0 = lattice_tile_first(tj, shift);
    // brute force: the corners of every cell whose tile this is
    std::set<long> want;
    for (int cj = j0; cj < j0 + W - 1; ++cj)
      for (int ci = i0; ci < i0 + W - 1; ++ci) {
        if (ci < -1 || ci > n1 || cj < -1 || cj > n2)
          continue;
        CHECK(lattice_tile_of(ci, shift) == ti && lattice_tile_of(cj, shift) == tj);
        for (int k = 0; k < 4; ++k)
          want.insert((long)(cj + (k >> 1)) * 100000L + (ci + (k & 1)));
      }
    std::set<int> slots;
    for (int j = j0 - 2; j <= j0 + W + 1; ++j)
      for (int i = i0 - 2; i <= i0 + W + 1; ++i) {
        const int s = lattice_tile_slot(i, j, ti, tj, shift);
        const bool in = i >= i0 && i < i0 + W && j >= j0 && j < j0 + W;
        CHECK((s >= 0) == in);
        if (s >= 0) {
          CHECK(s < W * W && s == (j - j0) * W + (i - i0));
          CHECK(slots.insert(s).second); // (no two indices share a slot)
        }
        if (want.count((long)j * 100000L + i))
          CHECK(s >= 0); // every corner of the tile's cells has a slot
      }
    CHECK((int)slots.size() == W * W);
  }
}

static void check_point(float u, float v, float phase1, float phase2, float delta, int n1, int n2, int shift) {
  const float invD = 1.f / delta;
  const int ci = lattice_lane_corner(u, phase1, invD, n1), cj = lattice_lane_corner(v, phase2, invD, n2);
  CHECK(ci >= -1 && ci <= n1 && cj >= -1 && cj <= n2);
  const int ti = lattice_tile_of(ci, shift), tj = lattice_tile_of(cj, shift);
  CHECK(ti >= 0 && ti < lattice_tiles_axis(n1, shift) && tj >= 0 && tj < lattice_tiles_axis(n2, shift));
  const int W = lattice_tile_width(shift);
  for (int k = 0; k < 4; ++k) {
    const int s = lattice_tile_slot(ci + (k & 1), cj + (k >> 1), ti, tj, shift);
    CHECK(s >= 0 && s < W * W);
  }
}

int main() {
  const int sizes[4] = {1, 2, 33, 1000};
  for (int shift = VR_TILE_SHIFT_MIN; shift <= VR_TILE_SHIFT_MAX; ++shift) {
    for (int n : sizes)
      check_axis(n, shift);
    for (int n1 : sizes)
      for (int n2 : sizes)
        check_slots(n1, n2, shift);
  }
  // (3) points: random ones, the table's border and beyond, the values no arithmetic should turn into an index
  std::mt19937 rng(20260117u);
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  for (int shift = VR_TILE_SHIFT_MIN; shift <= VR_TILE_SHIFT_MAX; ++shift)
    for (int n1 : sizes)
      for (int n2 : sizes)
        for (float delta : {1.f, 0.5f, 0.37f}) {
          const float phase1 = -0.5f * delta * (float)(n1 - 1), phase2 = 0.37f;
          const float e1 = delta * (float)(n1 - 1), e2 = delta * (float)(n2 - 1);
          std::uniform_real_distribution<float> U(-0.2f, 1.2f);
          for (int k = 0; k < 2000; ++k)
            check_point(phase1 + U(rng) * (e1 + delta), phase2 + U(rng) * (e2 + delta), phase1, phase2, delta, n1, n2, shift);
          // lattice lines, and the floats next to them
          for (int i : {0, 1, n1 - 2, n1 - 1, n1})
            for (int j : {0, 1, n2 - 2, n2 - 1, n2}) {
              const float x = phase1 + delta * (float)i, y = phase2 + delta * (float)j;
              for (float dx : {std::nextafterf(x, -inf), x, std::nextafterf(x, inf)})
                for (float dy : {std::nextafterf(y, -inf), y, std::nextafterf(y, inf)})
                  check_point(dx, dy, phase1, phase2, delta, n1, n2, shift);
            }
          for (float bad : {inf, -inf, nan, 3e38f, -3e38f})
            check_point(bad, phase2, phase1, phase2, delta, n1, n2, shift), check_point(phase1, bad, phase1, phase2, delta, n1, n2, shift);
        }
  // (4) sizing
  CHECK(lattice_tile_lds_bytes(VR_TILE_SHIFT_MAX) <= 160u * 1024u);
  CHECK(lattice_tile_lds_bytes(5) == 33u * 33u * 24u);
  CHECK((uint32_t)lattice_tiles_axis(1000, 6) * (uint32_t)lattice_tiles_axis(1000, 6) <= VR_TILE_MAX_TILES);
  CHECK((uint32_t)lattice_tiles_axis(1000, 5) * (uint32_t)lattice_tiles_axis(1000, 5) <= VR_TILE_MAX_TILES);
  uint32_t prev = 0;
  for (uint64_t rays : {1ull, 1000ull, 200000ull, 100000000ull, 134217728ull}) {
    const uint32_t cap = lattice_tile_capacity(rays, 64., 1000. * 1000.);
    CHECK(cap >= prev && (double)cap >= (double)rays * 4096. / 1e6 && (double)cap <= (double)rays + 1.);
    prev = cap;
    CHECK(lattice_tile_capacity(rays, 64., 0.) == (uint32_t)rays + 1u); // (no source area: room for every ray)
    CHECK(lattice_tile_capacity(rays, 64., 16.) == (uint32_t)rays + 1u); // (a tile larger than the source)
  }
  if (failed) {
    std::printf("lattice_tiles: %ld checks FAILED\n", failed);
    return 1;
  }
  std::printf("lattice_tiles: ok\n");
  return 0;
}
