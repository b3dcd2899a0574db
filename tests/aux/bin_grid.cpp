// bin_grid — host check of vr_bin_grid.hpp: the aligned sort-bin grid's rule and the float key against a double
// reference, over a table of domains.  Exit status 0: every row passes.  (tests/test_bin_grid_host.py builds and runs it.)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>

#include "../../viennaray_amd/csrc/vr_bin_grid.hpp"

using namespace vr;

struct Row {
  const char *name;
  float lo1, hi1, lo2, hi2, pitch, phase1, phase2;
  uint64_t rays;
  uint32_t perBin, binCap, ovCap;
  bool fallback; // the rule cannot be met here: the plain grid stays
};

static const Row rows[] = {
    // C2: 1000 x 1000 disks of pitch 1, 1e8 rays
    {"C2", -499.5f, 499.5f, -499.5f, 499.5f, 1.f, -499.5f, -499.5f, 100000000ull, 40, 128, 100000000u, false},
    {"C2 30 rays per disk", -499.5f, 499.5f, -499.5f, 499.5f, 1.f, -499.5f, -499.5f, 30000000ull, 40, 128, 30000000u, false},
    // the 40 x 40 plane at 1.25, 12.5 and 125 rays per lattice cell: sparse with m2 > 1, sparse with m2 = 1, dense with k2 > 1
    {"plane40 2e3", 0.f, 39.f, 0.f, 39.f, 1.f, 0.f, 0.f, 2000ull, 40, 128, 2000u, false},
    {"plane40 2e4", 0.f, 39.f, 0.f, 39.f, 1.f, 0.f, 0.f, 20000ull, 40, 128, 20000u, false},
    {"plane40 2e5", 0.f, 39.f, 0.f, 39.f, 1.f, 0.f, 0.f, 200000ull, 40, 128, 200000u, false},
    // T1 != T2, a partial tile on each axis
    {"40 x 24", 0.f, 39.f, 0.f, 23.f, 1.f, 0.f, 0.f, 100000ull, 40, 128, 100000u, false},
    // pitch and phase not trivial; the domain's lower end is the first centre
    {"pitch 0.7", 0.3f, 0.3f + 31 * 0.7f, -1.1f, -1.1f + 31 * 0.7f, 0.7f, 0.3f, -1.1f, 150000ull, 40, 128, 150000u, false},
    // the domain starts between two lattice lines (a cloud whose smallest centre is not on its edge)
    {"phase inside", -3.25f, 17.6f, 2.4f, 30.1f, 0.5f, 0.1f, 7.15f, 400000ull, 40, 128, 400000u, false},
    {"phase below", 10.f, 50.f, -20.f, 20.f, 1.f, -7.5f, -100.25f, 90000ull, 40, 128, 90000u, false},
    // more lattice cells than an axis may have cells: m >= 2 by the cap
    {"wide", 0.f, 9000.f, 0.f, 5000.f, 1.f, 0.f, 0.f, 100000000ull, 40, 128, 100000000u, false},
    // other knob values
    {"perBin 16 cap 64", 0.f, 99.f, 0.f, 99.f, 1.f, 0.f, 0.f, 1000000ull, 16, 64, 1000000u, false},
    {"perBin 200 cap 128", 0.f, 99.f, 0.f, 99.f, 1.f, 0.f, 0.f, 1000000ull, 200, 128, 1000000u, false},
    {"cap 8", 0.f, 99.f, 0.f, 99.f, 1.f, 0.f, 0.f, 1000000ull, 40, 8, 1000000u, false},
    // fall back: no lattice; a degenerate domain; bins that would have to be finer than the axis cap allows; a slot index
    // beyond 32 bits
    {"no pitch", 0.f, 99.f, 0.f, 99.f, 0.f, 0.f, 0.f, 1000000ull, 40, 128, 1000000u, true},
    {"flat domain", 0.f, 99.f, 5.f, 5.f, 1.f, 0.f, 5.f, 1000000ull, 40, 128, 1000000u, true},
    {"axis cap", 0.f, 2500.f, 0.f, 2500.f, 1.f, 0.f, 0.f, 134217728ull, 4, 16, 134217728u, true},
    {"slot index", -499.5f, 499.5f, -499.5f, 499.5f, 1.f, -499.5f, -499.5f, 134217728ull, 40, 2048, 134217728u, true},
};

static double ulpf(double x) { // spacing of the floats at |x|
  const float f = (float)std::fabs(x);
  return (double)std::nextafterf(f, INFINITY) - (double)f;
}

static bool near_integer(double x, double tol) { return std::fabs(x - std::floor(x + 0.5)) <= tol; }

int main() {
  int bad = 0;
  for (const Row &r : rows) {
    BinGridIn in;
    in.rays = r.rays;
    in.perBin = r.perBin;
    in.binCap = r.binCap;
    in.ovCap = r.ovCap;
    in.lo1 = r.lo1, in.hi1 = r.hi1, in.lo2 = r.lo2, in.hi2 = r.hi2;
    in.phase1 = r.phase1, in.phase2 = r.phase2;
    in.pitch = r.pitch;
    BinGrid g = bin_grid_plain(3, r.rays, r.perBin);
    const BinGrid plain = g;
    const bool ok = bin_grid_aligned(in, g);
    int fails = 0;
    auto check = [&](bool cond, const char *what) {
      if (!cond) {
        std::printf("  FAIL %s: %s\n", r.name, what);
        ++fails;
      }
    };
    check(ok == !r.fallback, r.fallback ? "the rule should fall back here" : "the rule should be met here");
    if (!ok) { // the plain grid is untouched
      check(g.aligned == 0 && g.T1 == plain.T1 && g.T2 == plain.T2 && g.numBins == plain.numBins && g.scale1 == plain.scale1 &&
                g.bias1 == 0.f && g.scale2 == plain.scale2 && g.bias2 == 0.f,
            "a refused rule leaves the plain grid as it was");
    }
    const double d = r.pitch, e1 = (double)r.hi1 - r.lo1, e2 = (double)r.hi2 - r.lo2;
    if (ok) {
      // the caps
      check(g.T1 >= 1 && g.T1 <= VR_BIN_AXIS_MAX && g.T2 >= 1 && g.T2 <= VR_BIN_AXIS_MAX, "cells per axis within the cap");
      check(g.tiles == (g.T1 + 7) / 8 && (uint64_t)g.numBins == (uint64_t)g.tiles * (uint64_t)((g.T2 + 7) / 8) * 64u, "numBins = tiles1 x tiles2 x 64");
      check((uint64_t)g.numBins * r.binCap + r.ovCap <= 0xFFFFFFFFull, "slot index fits 32 bits");
      // the edges: origin on a lattice line at or below lo (less than a cell below), cells of m or 1 / k lattice cells
      check(near_integer((g.origin1 - r.phase1) / d, 1e-9) && near_integer((g.origin2 - r.phase2) / d, 1e-9), "origin on a lattice line");
      check(g.origin1 <= r.lo1 + 2e-4 * d && r.lo1 - g.origin1 < d && g.origin2 <= r.lo2 + 2e-4 * d && r.lo2 - g.origin2 < d, "origin at or below lo");
      check(g.m1 >= 1 && g.m2 >= 1 && g.k2 >= 1 && (g.m2 == 1 || g.k2 == 1), "cell shape: integers");
      check(std::fabs(g.cell1 - d * g.m1) <= 1e-12 * d * g.m1 && std::fabs(g.cell2 - d * g.m2 / g.k2) <= 1e-12 * d * g.m2, "cells of m or 1 / k lattice cells");
      check(g.origin1 + g.T1 * g.cell1 >= r.hi1 - 1e-5 * g.cell1 && g.origin2 + g.T2 * g.cell2 >= r.hi2 - 1e-5 * g.cell2, "the cells cover the domain");
      check(g.origin1 + (g.T1 - 1) * g.cell1 < r.hi1 && g.origin2 + (g.T2 - 1) * g.cell2 < r.hi2, "no cell beyond the domain");
      // ... and the float mapping has them there: edge j at u = (j - bias) / scale, i.e. at lo + ext x u
      for (int ax = 0; ax < 2; ++ax) {
        const double sc = ax ? g.scale2 : g.scale1, bi = ax ? g.bias2 : g.bias1, lo = ax ? r.lo2 : r.lo1, e = ax ? e2 : e1;
        const double o = ax ? g.origin2 : g.origin1, cell = ax ? g.cell2 : g.cell1;
        const int T = ax ? g.T2 : g.T1;
        double worst = 0.;
        for (int j = 0; j <= T; ++j)
          worst = std::max(worst, std::fabs(lo + e * (j - bi) / sc - (o + j * cell)) / cell);
        check(worst <= 4.0 * T * 6e-8, "the float key's edges lie on the lattice (to the rounding of scale and bias)");
      }
      // mean rays per bin
      const double rho = (double)r.rays * d * d / (e1 * e2), mean = rho * g.m1 * g.m2 / g.k2;
      check(std::fabs(mean - g.meanRays) <= 1e-9 * mean, "meanRays");
      check(mean >= bin_grid_mean_lo(in) && mean <= bin_grid_mean_hi(in), "mean rays per bin within [min(perBin, binCap / 2) / 2, binCap / 2]");
    }
    // the key: 1e6 positions up to 2.5 extents outside the domain, under both wall folds (and none)
    std::mt19937_64 rng(12345);
    std::uniform_real_distribution<double> U(-2.5, 3.5);
    const float inv1 = e1 > 0. ? 1.f / (r.hi1 - r.lo1) : 0.f, inv2 = e2 > 0. ? 1.f / (r.hi2 - r.lo2) : 0.f;
    const double S1 = ok ? e1 / g.cell1 : (double)g.T1, B1 = ok ? ((double)r.lo1 - g.origin1) / g.cell1 : 0.;
    const double S2 = ok ? e2 / g.cell2 : (double)g.T2, B2 = ok ? ((double)r.lo2 - g.origin2) / g.cell2 : 0.;
    long outside = 0, wrong = 0, atEdge = 0;
    for (int s = 0; s < 1000000; ++s) {
      const float x = (float)(r.lo1 + U(rng) * e1), y = (float)(r.lo2 + U(rng) * e2);
      for (int bc = 0; bc < 3; ++bc) {
        const float u1 = fold_unit((x - r.lo1) * inv1, bc), u2 = fold_unit((y - r.lo2) * inv2, bc);
        const int c1 = bin_cell(u1, g.scale1, g.bias1, g.T1), c2 = bin_cell(u2, g.scale2, g.bias2, g.T2);
        const unsigned b = bin_index(c1, c2, g.tiles);
        if (c1 < 0 || c1 >= g.T1 || c2 < 0 || c2 >= g.T2 || b >= g.numBins)
          ++outside;
        const double x1 = (double)u1 * S1 + B1, x2 = (double)u2 * S2 + B2;
        const int cs[2] = {c1, c2}, Ts[2] = {g.T1, g.T2};
        const double xs[2] = {x1, x2};
        for (int ax = 0; ax < 2; ++ax) {
          int ref = (int)std::floor(xs[ax]);
          ref = ref < 0 ? 0 : (ref >= Ts[ax] ? Ts[ax] - 1 : ref);
          if (ref == cs[ax])
            continue;
          const double edge = std::floor(xs[ax] + 0.5);
          if (std::abs(ref - cs[ax]) == 1 && std::fabs(xs[ax] - edge) <= 2. * ulpf(std::max(1., std::max(std::fabs(xs[ax]), edge))))
            ++atEdge;
          else
            ++wrong;
        }
      }
    }
    check(outside == 0, "every cell inside [0, T), every bin below numBins");
    check(wrong == 0, "float cell == double cell except within 2 ulp of an edge");
    std::printf("%-20s %s  %d x %d cells (m1 %d m2 %d k2 %d), %u bins, mean %.1f rays per bin; key: %ld at an edge, %ld wrong, %ld outside%s\n",
                r.name, ok ? "aligned" : "plain  ", g.T1, g.T2, g.m1, g.m2, g.k2, g.numBins, g.meanRays, atEdge, wrong, outside,
                fails ? "  FAILED" : "");
    bad += fails;
  }
  std::printf("%d failed checks\n", bad);
  return bad ? 1 : 0;
}
