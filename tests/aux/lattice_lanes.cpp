// Four corners per lane (vr_planar_lattice.hpp: lattice_lanes_rule, lattice_lane_corner, lattice_window_slot) on the host,
// against a brute force over every disk of the lattice.
// (a) corner containment: lattices of pitch 1, 0.5 and 0.37 at phases 0, 0.37 and -499.5, radii at the rule's limit and
//     just below it, every centre jittered by up to exactly delta / 8 (as far as lattice_cell_of files it), points that are
//     random, on lattice lines and within +-4 ulp of them, at the table's first and last row and column, and non-finite:
//     every disk that planar_round_cand accepts for hit or local — found by testing ALL disks — is one of the four corners
//     of the cell lattice_lane_corner names, every corner index is inside the table or flagged absent, and for a point in
//     a round's box the accepting disk's window slot is the lane that lattice_lane_cell gives that cell.
// (b) the rule: it refuses a radius one ulp above its limit and a scene moved so far from the origin that 12 ulp of the
//     largest coordinate eat the margin, and takes the headline scene's numbers (1000 x 1000, pitch 1, radius 0.866).
// `lattice_lanes offset <delta> <radius> <n>`: the smallest power-of-two offset of an n x n lattice from the origin at which
// the rule refuses it (tests/test_lattice_lanes.py builds its scene (o) from that number).
// Plain C++17, vr_planar_lattice.hpp and vr_planar_disks.hpp alone.  tests/test_lattice_lanes_host.py reads the last lines.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "vr_planar_disks.hpp"
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

// the largest radius the rule takes at this pitch and coordinate bound (the rule is monotone in the radius)
static float limit_radius(float delta, float C) {
  float lo = 0.25f * delta, hi = delta;
  if (!lattice_lanes_rule(lo, delta, C))
    return 0.f;
  while (std::nextafter(lo, hi) < hi) {
    const float mid = lo + 0.5f * (hi - lo);
    (lattice_lanes_rule(mid, delta, C) ? lo : hi) = mid;
  }
  return lo;
}
static float step(float x, int ulps) {
  for (int s = 0; s < std::abs(ulps); ++s)
    x = std::nextafter(x, ulps > 0 ? std::numeric_limits<float>::infinity() : -std::numeric_limits<float>::infinity());
  return x;
}
// the smallest power-of-two offset at which an n x n lattice of this pitch and radius is refused (centres alone bound the
// scene here: the scene box of a launch is no smaller, and the rule only gets stricter with a larger coordinate)
static float refusing_offset(float delta, float radius, int n) {
  for (int e = 0; e < 60; ++e) {
    const float off = std::ldexp(1.f, e);
    if (!lattice_lanes_rule(radius, delta, lattice_lanes_coord(off + (float)(n - 1) * delta, delta)))
      return off;
  }
  return 0.f;
}

int main(int argc, char **argv) {
  if (argc == 5 && !std::strcmp(argv[1], "offset")) {
    std::printf("%.9g\n", (double)refusing_offset((float)std::atof(argv[2]), (float)std::atof(argv[3]), std::atoi(argv[4])));
    return 0;
  }
  std::mt19937_64 g(20250117u);
  std::uniform_real_distribution<double> U(0., 1.);
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();

  // ---- (a) corner containment
  long clouds = 0, points = 0, accepted = 0, onLines = 0, absent = 0, nonFinite = 0, edgeCentres = 0, slots = 0;
  const int n1 = 11, n2 = 9;
  for (float delta : {1.f, 0.5f, 0.37f})
    for (float phase : {0.f, 0.37f, -499.5f})
      for (int rad = 0; rad < 3; ++rad) {
        const float ph[2] = {phase, phase == 0.f ? 0.37f : phase}; // (the two axes need not share a phase)
        const int nn[2] = {n1, n2};
        const float invD = 1.f / delta;
        // centres: jitter up to exactly delta / 8 per axis, pulled back ulp by ulp where lattice_cell_of would not file it
        std::vector<float> cu((size_t)n1 * n2), cv((size_t)n1 * n2);
        float maxAbs = 0.f;
        for (int i = 0; i < n1; ++i)
          for (int j = 0; j < n2; ++j) {
            const int idx[2] = {i, j};
            float c[2];
            for (int a = 0; a < 2; ++a) {
              const int m = (int)(4 * U(g));
              const double jit = m == 0 ? 0.125 : m == 1 ? -0.125 : -0.125 + 0.25 * U(g);
              const double x = (double)ph[a] + (double)idx[a] * (double)delta;
              c[a] = (float)(x + jit * (double)delta);
              int k;
              bool pulled = false;
              // (phase is the smallest centre coordinate: no centre below the first lattice line)
              if (idx[a] == 0 && c[a] < ph[a])
                c[a] = ph[a];
              while (!lattice_cell_of(c[a], ph[a], invD, nn[a], k)) {
                c[a] = std::nextafter(c[a], (float)x);
                pulled = true;
              }
              CHECK(k == idx[a]);
              edgeCentres += pulled || m < 2;
              maxAbs = std::fmax(maxAbs, std::fabs(c[a]));
            }
            cu[(size_t)i * n2 + j] = c[0];
            cv[(size_t)i * n2 + j] = c[1];
          }
        const float C = lattice_lanes_coord(maxAbs, delta);
        const float rLimit = limit_radius(delta, C);
        CHECK(rLimit > 0.8f * delta && lattice_lanes_rule(rLimit, delta, C) && !lattice_lanes_rule(std::nextafter(rLimit, inf), delta, C));
        const float radius = rad == 0 ? rLimit : rad == 1 ? step(rLimit, -3) : 0.8660254f * delta * 0.99f;
        CHECK(lattice_lanes_rule(radius, delta, C));
        ++clouds;
        const float ca = 0.25f;
        const float pad = 1e-5f * (maxAbs + radius);
        const float reach = lattice_reach(radius, delta, pad);
        auto test_point = [&](float u, float v) {
          ++points;
          nonFinite += !(std::isfinite(u) && std::isfinite(v));
          PlanarRound r;
          r.t = 1.f;
          r.qx = u, r.qy = v, r.qz = ca;
          r.hitThr = radius * radius; // (both tests at their widest: the neighbour test's threshold is at most this)
          r.locThr = radius * radius;
          const int ci = lattice_lane_corner(u, ph[0], invD, n1), cj = lattice_lane_corner(v, ph[1], invD, n2);
          CHECK(ci >= -1 && ci <= n1 && cj >= -1 && cj <= n2);
          for (int k = 0; k < 4; ++k) // (a corner is a lattice point, or flagged absent: nothing else)
            absent += !(ci + (k & 1) >= 0 && ci + (k & 1) < n1 && cj + (k >> 1) >= 0 && cj + (k >> 1) < n2);
          // the window of a round whose box is this point alone
          int i0, i1, j0, j1;
          lattice_axis_window(u - pad, u + pad, ph[0], invD, reach, n1, i0, i1);
          lattice_axis_window(v - pad, v + pad, ph[1], invD, reach, n2, j0, j1);
          const int w = i1 - i0 + 1, rows = j1 - j0 + 1;
          for (int i = 0; i < n1; ++i)
            for (int j = 0; j < n2; ++j) {
              bool hit, local;
              planar_round_cand(r, cu[(size_t)i * n2 + j], cv[(size_t)i * n2 + j], ca, hit, local);
              if (!(hit || local))
                continue;
              ++accepted;
              CHECK((i == ci || i == ci + 1) && (j == cj || j == cj + 1));
              // ... and inside the window, in the slot of the lane that files that cell
              CHECK(w >= 1 && rows >= 1 && w * rows <= VR_LATTICE_WINDOW);
              const int s = lattice_window_slot(i, j, i0, i1, j0, j1);
              CHECK(s >= 0 && s < w * rows && s < VR_LATTICE_WINDOW);
              if (s >= 0 && w >= 1) {
                int col, row;
                lattice_lane_cell(s, w, 1.f / (float)w, col, row);
                CHECK(i0 + col == i && j0 + row == j);
                ++slots;
              }
            }
          // every slot the function hands out is a cell of the window, and the window a part of the table
          for (int k = 0; k < 4; ++k) {
            const int s = lattice_window_slot(ci + (k & 1), cj + (k >> 1), i0, i1, j0, j1);
            CHECK(s >= -1 && (s < 0 || (w >= 1 && rows >= 1 && s < w * rows && i0 >= 0 && i1 < n1 && j0 >= 0 && j1 < n2)));
          }
        };
        // random points, from two cells outside the lattice to two cells beyond it
        for (int k = 0; k < 6000; ++k)
          test_point((float)((double)ph[0] + delta * (-2. + (n1 + 3.) * U(g))), (float)((double)ph[1] + delta * (-2. + (n2 + 3.) * U(g))));
        // on lattice lines and within +-4 ulp of them (one axis, both axes), the first and the last line included
        for (int i = -1; i <= n1; ++i)
          for (int du = -4; du <= 4; ++du) {
            const float u = step((float)((double)ph[0] + (double)i * (double)delta), du);
            for (int j = -1; j <= n2; ++j) {
              test_point(u, step((float)((double)ph[1] + (double)j * (double)delta), (int)(9 * U(g)) - 4));
              test_point(u, (float)((double)ph[1] + delta * (-1. + (n2 + 1.) * U(g))));
              test_point((float)((double)ph[0] + delta * (-1. + (n1 + 1.) * U(g))), step((float)((double)ph[1] + (double)j * (double)delta), du));
              onLines += 3;
            }
          }
        // as close to a disk's edge as floats get, from a centre towards each neighbouring cell
        for (int k = 0; k < 400; ++k) {
          const size_t d = (size_t)(U(g) * n1 * n2);
          const double ang = 6.283185307179586 * U(g);
          test_point((float)(cu[d] + (double)radius * std::cos(ang) * (1. - 1e-7 * U(g))), (float)(cv[d] + (double)radius * std::sin(ang) * (1. - 1e-7 * U(g))));
        }
        // non-finite and huge points
        for (float u : {nan, inf, -inf, 3e38f, -3e38f, 1e9f, ph[0] + 2.f * delta})
          for (float v : {nan, inf, -inf, 3e38f, -1e9f, ph[1] + 3.f * delta})
            test_point(u, v);
      }
  std::printf("%ld clouds, %ld points (%ld on or beside lattice lines, %ld not finite or huge), %ld accepting disks, %ld absent corners, "
              "%ld centres at the tolerance's edge, %ld window slots\n",
              clouds, points, onLines, nonFinite, accepted, absent, edgeCentres, slots);

  // ---- (b) the rule
  {
    // the headline scene: 1000 x 1000 at pitch 1, centres -499.5 .. 499.5, radius 0.866 delta, scene box +- (499.5 + r)
    const float C2 = lattice_lanes_coord(499.5f + 0.8660254f, 1.f);
    CHECK(lattice_lanes_rule(0.8660254f, 1.f, C2));
    CHECK(lattice_lanes_rule(0.8660254f * 0.5f, 0.5f, 20.f) && lattice_lanes_rule(0.8660254f * 0.37f, 0.37f, 20.f));
    const float rl = limit_radius(1.f, C2);
    CHECK(rl > 0.87f && rl < 0.875f);
    CHECK(lattice_lanes_rule(rl, 1.f, C2) && !lattice_lanes_rule(std::nextafter(rl, 2.f), 1.f, C2));
    // a coordinate offset that eats the margin: 12 ulp of C against 0.009 delta
    const float off = refusing_offset(1.f, 0.8660254f, 32);
    CHECK(off >= 1024.f && off <= 65536.f);
    CHECK(!lattice_lanes_rule(0.8660254f, 1.f, lattice_lanes_coord(off + 31.f, 1.f)));
    CHECK(lattice_lanes_rule(0.8660254f, 1.f, lattice_lanes_coord(0.5f * off + 31.f, 1.f)));
    // nonsense in: refused
    CHECK(!lattice_lanes_rule(0.f, 1.f, 10.f) && !lattice_lanes_rule(0.5f, 0.f, 10.f) && !lattice_lanes_rule(nan, 1.f, 10.f) &&
          !lattice_lanes_rule(0.5f, 1.f, nan) && !lattice_lanes_rule(0.5f, 1.f, inf) && !lattice_lanes_rule(1.f, 1.f, 10.f));
    std::printf("rule: limit radius %.9g at pitch 1 (headline scene), refusing offset %.9g\n", (double)rl, (double)off);
  }
  std::printf("%ld failed checks\n", failed);
  return failed ? 1 : 0;
}
