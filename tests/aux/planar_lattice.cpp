// The lattice table's arithmetic (vr_planar_lattice.hpp) on the host, against a double-precision brute force.
// (1) the window: over random boxes, phases, pitches (1, 0.5, 0.37 and random ones), radii and centres jittered by up to
//     delta / 8, every lattice disk whose ball meets the padded box — in double, and by the kernel's float filter — lies inside
//     lattice_axis_window's indices, and the window never leaves the table (also for boxes far outside it and NaNs);
// (2) lattice_lane_cell is l % w, l / w for every lane, every width and a reciprocal an ulp or two off;
// (3) the table rule (lattice_axis_points, lattice_table_fits, lattice_cell_of with the kernel's claim of a cell) takes a
//     32 x 48 lattice, one with a hole, one with every centre jittered by 0.05 delta, pitch 0.5 and phase 0.37, and refuses a
//     centre moved by 0.3 delta, two disks in one cell and n1 n2 > 4 N.
// Plain C++17, vr_planar_lattice.hpp alone.  tests/test_planar_lattice_host.py reads the last lines.
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

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

// ---- (3) the table as launch_lattice_table builds it: flags bit 0 off the lattice, bit 1 two disks at one point; -1: no table
struct Cloud {
  std::vector<float> u, v;
  float delta;
};
static int build_table(const Cloud &c, std::vector<uint32_t> &table, int &n1, int &n2) {
  float lo1 = c.u[0], hi1 = c.u[0], lo2 = c.v[0], hi2 = c.v[0];
  for (size_t k = 0; k < c.u.size(); ++k) {
    lo1 = std::fmin(lo1, c.u[k]), hi1 = std::fmax(hi1, c.u[k]);
    lo2 = std::fmin(lo2, c.v[k]), hi2 = std::fmax(hi2, c.v[k]);
  }
  n1 = lattice_axis_points(lo1, hi1, c.delta);
  n2 = lattice_axis_points(lo2, hi2, c.delta);
  if (!lattice_table_fits(n1, n2, (uint32_t)c.u.size()))
    return -1;
  table.assign((size_t)n1 * n2, VR_LATTICE_EMPTY);
  const float invD = 1.f / c.delta;
  int flags = 0;
  for (size_t k = 0; k < c.u.size(); ++k) {
    int i, j;
    const bool on1 = lattice_cell_of(c.u[k], lo1, invD, n1, i), on2 = lattice_cell_of(c.v[k], lo2, invD, n2, j);
    CHECK(i >= 0 && i < n1 && j >= 0 && j < n2); // (whatever the verdict: an index inside the table)
    if (!(on1 && on2))
      flags |= 1;
    else if (table[(size_t)j * n1 + i] != VR_LATTICE_EMPTY)
      flags |= 2;
    else
      table[(size_t)j * n1 + i] = (uint32_t)k;
  }
  return flags;
}
static Cloud lattice(int a, int b, float delta, float phase1, float phase2, float jitter, std::mt19937 &g) {
  Cloud c;
  c.delta = delta;
  std::uniform_real_distribution<float> J(-jitter, jitter);
  for (int i = 0; i < a; ++i)
    for (int j = 0; j < b; ++j) {
      c.u.push_back(phase1 + (float)i * delta + (jitter > 0.f ? J(g) * delta : 0.f));
      c.v.push_back(phase2 + (float)j * delta + (jitter > 0.f ? J(g) * delta : 0.f));
    }
  return c;
}

int main() {
  std::mt19937 g(20240611u);
  std::mt19937_64 g64(77u);
  std::uniform_real_distribution<double> U(0., 1.);
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();

  // ---- (1) the window
  long cases = 0, disks = 0, meeting = 0, clamped = 0, empty = 0, edge = 0;
  for (int trial = 0; trial < 20000; ++trial) {
    const int pick = trial % 4;
    const float delta = pick == 0 ? 1.f : pick == 1 ? 0.5f : pick == 2 ? 0.37f : (float)(0.1 + 2.9 * U(g64));
    const float phase1 = trial % 3 == 0 ? 0.37f : (float)(-500. + 1000. * U(g64)), phase2 = trial % 5 == 0 ? -15.5f : (float)(-500. + 1000. * U(g64));
    const int n1 = 1 + (int)(60 * U(g64)), n2 = 1 + (int)(60 * U(g64));
    const float radius = trial % 7 == 0 ? delta * 0.8660340f : (float)(delta * (0.2 + 1.3 * U(g64)));
    const float invD = 1.f / delta;
    float scale = 1e-3f;
    for (float e : {phase1, phase2, phase1 + n1 * delta, phase2 + n2 * delta})
      scale = std::fmax(scale, std::fabs(e) + radius);
    const float pad = 1e-5f * scale;
    const float reach = lattice_reach(radius, delta, pad);
    // the box of some plane hits: anywhere from three cells outside the lattice to three cells beyond it, up to three cells wide
    float lo[2], hi[2];
    const float ph[2] = {phase1, phase2};
    const int nn[2] = {n1, n2};
    for (int a = 0; a < 2; ++a) {
      const double x = ph[a] + delta * (-3. + (nn[a] + 5.) * U(g64)), wdt = trial % 11 == 0 ? 0. : delta * 3. * U(g64);
      lo[a] = (float)x - pad;
      hi[a] = (float)(x + wdt) + pad;
    }
    int k0[2], k1[2];
    for (int a = 0; a < 2; ++a) {
      lattice_axis_window(lo[a], hi[a], ph[a], invD, reach, nn[a], k0[a], k1[a]);
      CHECK(k0[a] >= 0 && k0[a] <= nn[a] && k1[a] >= -1 && k1[a] <= nn[a] - 1);
      if (k0[a] <= k1[a])
        CHECK(k0[a] >= 0 && k1[a] <= nn[a] - 1); // the window never leaves the table
      else
        ++empty;
      clamped += (k0[a] == 0 || k1[a] == nn[a] - 1);
    }
    ++cases;
    for (int i = 0; i < n1; ++i)
      for (int j = 0; j < n2; ++j) {
        const int idx[2] = {i, j};
        float c[2];
        bool meetsD = true, meetsF = true;
        for (int a = 0; a < 2; ++a) {
          const int m = (int)(5 * U(g64));
          const double jit = m == 0 ? 0.125 : m == 1 ? -0.125 : -0.125 + 0.25 * U(g64); // (also exactly delta / 8)
          c[a] = (float)((double)ph[a] + (double)idx[a] * (double)delta + jit * (double)delta);
          meetsD = meetsD && (double)c[a] - (double)radius <= (double)hi[a] && (double)c[a] + (double)radius >= (double)lo[a];
          meetsF = meetsF && c[a] - radius <= hi[a] && c[a] + radius >= lo[a]; // (the kernel's ball-box filter)
          int k;
          if (lattice_cell_of(c[a], ph[a], invD, nn[a], k)) // (at the edge of the tolerance the rule may refuse; it never misfiles)
            CHECK(k == idx[a]);
          else
            ++edge;
        }
        ++disks;
        if (meetsD || meetsF) {
          ++meeting;
          CHECK(i >= k0[0] && i <= k1[0] && j >= k0[1] && j <= k1[1]);
        }
      }
  }
  // boxes far outside the table, infinite ones and NaNs: an empty or a clamped window, never an index outside
  for (float lo : {-3e38f, -1e9f, -7.f, 0.f, 40.f, 1e9f, 3e38f, inf, -inf, nan})
    for (float hi : {-3e38f, -1e9f, 0.f, 12.f, 1e9f, 3e38f, inf, -inf, nan})
      for (int n : {1, 2, 33, VR_LATTICE_MAX_AXIS}) {
        int k0, k1;
        lattice_axis_window(lo, hi, 0.37f, 2.f, 0.9f, n, k0, k1);
        CHECK(k0 >= 0 && k0 <= n && k1 >= -1 && k1 <= n - 1);
      }
  std::printf("%ld window cases: %ld disks, %ld of them meeting the box, %ld clamped ends, %ld empty windows, %ld centres at the tolerance's edge\n",
              cases, disks, meeting, clamped, empty, edge);

  // ---- (2) a lane's cell
  long lanes = 0;
  for (int w = 1; w <= 64; ++w)
    for (int ulp = -2; ulp <= 2; ++ulp) {
      float inv = 1.f / (float)w;
      for (int s = 0; s < std::abs(ulp); ++s)
        inv = std::nextafter(inv, ulp > 0 ? 2.f : 0.f);
      for (int l = 0; l < 64; ++l) {
        int col, row;
        lattice_lane_cell(l, w, inv, col, row);
        CHECK(row == l / w && col == l % w);
        ++lanes;
      }
    }
  std::printf("%ld lane cells\n", lanes);

  // ---- (3) the table rule
  std::vector<uint32_t> table;
  int n1, n2, taken = 0, refused = 0;
  {
    Cloud c = lattice(32, 48, 1.f, -15.5f, -23.5f, 0.f, g);
    CHECK(build_table(c, table, n1, n2) == 0 && n1 == 32 && n2 == 48);
    for (int i = 0; i < 32; ++i)
      for (int j = 0; j < 48; ++j)
        CHECK(table[(size_t)j * n1 + i] == (uint32_t)(i * 48 + j)); // [n2][n1]: no row / column swap
    ++taken;
    Cloud moved = c;
    moved.u[17 * 48 + 5] += 0.3f; // one centre 0.3 delta off its lattice point
    CHECK(build_table(moved, table, n1, n2) == 1);
    ++refused;
    Cloud twice = c;
    twice.u.push_back(c.u[100]), twice.v.push_back(c.v[100]); // two disks in one cell
    CHECK(build_table(twice, table, n1, n2) == 2);
    ++refused;
    Cloud hole = c; // (holes are allowed: their cells stay empty)
    hole.u.erase(hole.u.begin() + 500, hole.u.begin() + 536), hole.v.erase(hole.v.begin() + 500, hole.v.begin() + 536);
    CHECK(build_table(hole, table, n1, n2) == 0 && n1 == 32 && n2 == 48);
    long emptyCells = 0;
    for (uint32_t w : table)
      emptyCells += w == VR_LATTICE_EMPTY;
    CHECK(emptyCells == 36);
    ++taken;
  }
  for (float delta : {1.f, 0.5f, 0.37f}) {
    Cloud c = lattice(40, 25, delta, 0.37f, -3.25f, 0.05f, g); // every centre jittered by up to 0.05 delta: still a lattice cloud
    CHECK(build_table(c, table, n1, n2) == 0 && n1 == 40 && n2 == 25);
    ++taken;
  }
  {
    Cloud c; // ten disks on a diagonal: 10 x 10 points for 10 disks
    c.delta = 1.f;
    for (int k = 0; k < 10; ++k)
      c.u.push_back((float)k), c.v.push_back((float)k);
    CHECK(build_table(c, table, n1, n2) == -1 && n1 == 10 && n2 == 10);
    ++refused;
    CHECK(lattice_table_fits(10, 4, 10) && !lattice_table_fits(10, 4, 9) && !lattice_table_fits(0, 4, 10) && !lattice_table_fits(4, 4, 0));
    CHECK(lattice_axis_points(0.f, 1e9f, 1.f) == 0 && lattice_axis_points(0.f, 1.f, 0.f) == 0 && lattice_axis_points(0.f, nan, 1.f) == 0 &&
          lattice_axis_points(2.f, 2.f, 1.f) == 1 && lattice_axis_points(-499.5f, 499.5f, 1.f) == 1000);
    // the window of a one-cell box in 64 lanes: the reference's disk radius does, a disk five cells wide does not
    CHECK(lattice_window_pays(lattice_reach(0.8660340f, 1.f, 5e-3f), 1.f) && !lattice_window_pays(lattice_reach(5.f, 1.f, 5e-3f), 1.f));
  }
  std::printf("table rule: %d clouds taken, %d refused\n", taken, refused);
  std::printf("%ld failed checks\n", failed);
  return failed ? 1 : 0;
}
