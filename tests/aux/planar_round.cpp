// The one-point-per-round forms of the planar-disk tests (viennaray_amd/csrc/vr_planar_disks.hpp (1) - (3)) on the host.
// Compiled with -ffp-contract=off -fno-fast-math like the library: the same operations in the same order as on the device.
//
// (1) planar_round_point / planar_round_cand against planar_hit_round / planar_hit_cand and planar_local_round /
//     planar_local_cand (which tests/aux/planar_disks.cpp ties to hit_disc_uniform / local_disc_hit_uniform): the same two
//     decisions in every case, the same bits of t wherever the hit test accepts, both refused for a lane that takes no
//     part.  Operands as in planar_disks.cpp: zeros of both signs, denormals, origins on the plane, zero and tiny
//     directions along the axis, non-finite origins, t near tnear.
// (2) the box: for a lane that counts (planar_round_valid, with the scene box the disk's own padded box: the tightest
//     there is) and a centre either test accepts, the ball filter of pq_hit_packet (c - r <= hi, c + r >= lo per
//     coordinate) passes on the box of that lane's point ALONE, q -+ pad in the plane and ca -+ pad along the axis — the hull
//     over a wave's lanes only grows it.  Centres at the acceptance edge (|q - c| = r up to a few ulp) are half the cases;
//     clouds near the origin and 1000 units off it.
// (3) the wall rule: rectangles of every proportion of offset to extent up to the rule's limit of 1000 and beyond it
//     (beyond: planar_wall_inner must hand out an empty rectangle); origins inside, exactly on a wall, one ulp outside;
//     points aimed at the shrunk rectangle's edge, one ulp inside and outside it.  Required for every lane the rule calls
//     wall-free with a plane hit (hitThr > 0): for all four walls the pre-tests of hit_walls_from (restated below) reject
//     in float — not reachable, or tw > fl(t * 1.001f) — with the reciprocal 1 / d correctly rounded and one ulp off
//     either way (the device's is approximate), and in double the wall's parameter is at least 1.0017 t.
// Prints the counts and "N failed checks"; exit status 1 if N > 0.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>

#include "../../viennaray_amd/csrc/vr_planar_disks.hpp"
#include "../../viennaray_amd/csrc/vr_uniform_disks.hpp"

static const int CASES_PER_CONFIG = 60000;
static const int WALL_CASES = 3000000;

static float from_bits(uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
static uint32_t to_bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}
static float edot(const float *a, const float *b) { return a[0] * b[0] + (a[1] * b[1] + a[2] * b[2]); }
static float vdot(const float *a, const float *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
static float up(float v) { return std::nextafter(v, std::numeric_limits<float>::infinity()); }
static float down(float v) { return std::nextafter(v, -std::numeric_limits<float>::infinity()); }

struct Gen {
  std::mt19937_64 rng{20261019ull};
  uint32_t u32() { return (uint32_t)(rng() >> 32); }
  float unit() { return (float)(u32() >> 8) * (1.f / 16777216.f); } // [0, 1)
  float sym(float a) { return (2.f * unit() - 1.f) * a; }
  float denormal() { return from_bits((u32() & 0x807FFFFFu) | 1u); }
  float coord(float a) {
    const uint32_t k = u32() % 16u;
    if (k == 0u)
      return 0.f;
    if (k == 1u)
      return -0.f;
    if (k == 2u)
      return denormal();
    return sym(a);
  }
  float nonfinite() {
    const uint32_t k = u32() % 3u;
    const float inf = std::numeric_limits<float>::infinity();
    return k == 0u ? inf : (k == 1u ? -inf : std::numeric_limits<float>::quiet_NaN());
  }
};

// hit_walls_from's pre-tests for one wall (vr_intersect.hpp): true where the wall goes on to its triangle tests
static bool wall_passes(float W, float oa, float da, float rcp, float tLimit) {
  const float c = W - oa;
  if (!((c > 0.f && da > 0.f) || (c < 0.f && da < 0.f))) // (wall_reachable)
    return false;
  const float tw = (W - oa) * rcp;
  return !(tw > tLimit);
}

int main() {
  const float tnear = 1e-4f;
  Gen g;
  unsigned long long failed = 0;

  // ---- (1) one point for both tests, (2) the box from it ----------------------------------------------------------
  const float heights[4] = {0.f, -0.f, 0.3f, -7.25f};
  const float radii[3] = {0.8660254f, 0.43301272f, 1.0f};
  unsigned long long cases = 0, hitAccepts = 0, localAccepts = 0, nearTnear = 0, boxChecks = 0, edgeAccepts = 0;
  for (int hi = 0; hi < 4; ++hi)
    for (int si = 0; si < 2; ++si)
      for (int a = 0; a < 3; ++a)
        for (int zp = 0; zp < 4; ++zp)
          for (int far = 0; far < 2; ++far) {
            const float ca = heights[hi], s = si ? -1.f : 1.f;
            int b1, b2;
            vr::planar_in_plane_axes(a, b1, b2);
            if (b1 == a || b2 == a || b1 >= b2) {
              std::printf("  planar_in_plane_axes(%d) gives %d, %d\n", a, b1, b2);
              ++failed;
            }
            const float shift = far ? 1000.f : 0.f; // the cloud's place in the plane
            float n[3];
            n[a] = s;
            n[b1] = (zp & 1) ? -0.f : 0.f;
            n[b2] = (zp & 2) ? -0.f : 0.f;
            for (int k = 0; k < CASES_PER_CONFIG; ++k) {
              float o[3], d[3], c[3];
              for (int j = 0; j < 3; ++j) {
                o[j] = g.coord(8.f) + (j == a ? 0.f : shift);
                d[j] = g.coord(1.f);
              }
              const uint32_t ko = g.u32() % 8u;
              if (ko == 0u)
                o[a] = ca;
              else if (ko <= 4u)
                o[a] = ca + s * (0.01f + 4.f * g.unit());
              const uint32_t kd = g.u32() % 16u;
              if (kd == 0u)
                d[a] = (g.u32() & 1u) ? 0.f : -0.f;
              else if (kd == 1u)
                d[a] = g.sym(2e-6f);
              else if (kd == 2u)
                d[a] = g.denormal();
              else if (kd <= 10u)
                d[a] = -s * (0.05f + g.unit());
              if (ko == 5u) { // t within a few ulp of tnear, on either side
                d[a] = -s * (0.05f + g.unit());
                o[a] = ca - d[a] * tnear * (1.f + g.sym(4e-7f));
                ++nearTnear;
              }
              if (g.u32() % 32u == 0u)
                o[g.u32() % 3u] = g.nonfinite();
              const float radius = radii[g.u32() % 3u], thresh = vr::uniform_disk_threshold(radius);
              c[a] = ca;
              c[b1] = g.coord(8.f) + shift;
              c[b2] = g.coord(8.f) + shift;
              bool edge = false;
              if (g.u32() & 1u) {
                const double t = ((double)ca - (double)o[a]) / (double)d[a];
                const double h1 = (double)o[b1] + (double)d[b1] * t, h2 = (double)o[b2] + (double)d[b2] * t;
                if (std::isfinite(h1) && std::isfinite(h2) && std::fabs(h1) < 1e6 && std::fabs(h2) < 1e6) {
                  if (g.u32() & 1u) { // at the acceptance edge: |q - c| = r up to the rounding
                    const double phi = 6.283185307179586 * g.unit(), rr = (double)radius * (1.0 + g.sym(3e-7f));
                    c[b1] = (float)(h1 + rr * std::cos(phi));
                    c[b2] = (float)(h2 + rr * std::sin(phi));
                    edge = true;
                  } else {
                    c[b1] = (float)h1 + g.sym(1.2f);
                    c[b2] = (float)h2 + g.sym(1.2f);
                  }
                }
              }
              const float divisor = edot(d, n), prod = vdot(n, d), nro = vdot(n, o);
              const vr::PlanarHit ph = vr::planar_hit_round(true, o[0], o[1], o[2], d[0], d[1], d[2], o[a], tnear, ca, s, divisor);
              const vr::PlanarLocal pl = vr::planar_local_round(true, o[0], o[1], o[2], d[0], d[1], d[2], ca, s, prod, nro);
              const bool hitRef = vr::planar_hit_cand(ph, c[0], c[1], c[2], radius);
              const bool locRef = vr::planar_local_cand(pl, c[0], c[1], c[2], thresh);
              const vr::PlanarRound pr =
                  vr::planar_round_point(true, o[0], o[1], o[2], d[0], d[1], d[2], o[a], d[a] * s, tnear, ca, s, radius, thresh);
              bool hitNew, locNew;
              vr::planar_round_cand(pr, c[0], c[1], c[2], hitNew, locNew);
              bool bad = hitNew != hitRef || locNew != locRef || (hitRef && to_bits(pr.t) != to_bits(ph.t));
              if ((k & 15) == 0) { // a lane that takes no part
                const vr::PlanarRound p0 =
                    vr::planar_round_point(false, o[0], o[1], o[2], d[0], d[1], d[2], o[a], d[a] * s, tnear, ca, s, radius, thresh);
                bool h0, l0;
                vr::planar_round_cand(p0, c[0], c[1], c[2], h0, l0);
                bad = bad || h0 || l0 || p0.hitThr != 0.f || p0.locThr != 0.f;
              }
              if (bad) {
                if (failed < 10)
                  std::printf("  (1) ca %g s %g axis %d zeros %d: o (%.9g %.9g %.9g) d (%.9g %.9g %.9g) c (%.9g %.9g %.9g) r %.9g: hit %d/%d t %08x/%08x local %d/%d\n",
                              ca, s, a, zp, o[0], o[1], o[2], d[0], d[1], d[2], c[0], c[1], c[2], radius, (int)hitRef, (int)hitNew,
                              to_bits(ph.t), to_bits(pr.t), (int)locRef, (int)locNew);
                ++failed;
              }
              hitAccepts += hitRef;
              localAccepts += locRef;
              ++cases;
              // (2): a centre that either test accepts, for a lane that can hit
              if ((hitNew || locNew) && pr.hitThr > 0.f) {
                const float q[3] = {pr.qx, pr.qy, pr.qz};
                // the scales as the library takes them: the largest coordinate of the scene box (here: of this disk's box)
                float scale = 1e-3f;
                for (int j = 0; j < 3; ++j)
                  scale = std::fmax(scale, std::fabs(c[j]) + (j == a ? 0.f : radius * 1.0001f));
                const float pad = 1e-5f * scale, boxPad = 4e-6f * scale;
                const float sLo1 = ((c[b1] - radius * 1.0001f) - boxPad) - pad, sHi1 = ((c[b1] + radius * 1.0001f) + boxPad) + pad;
                const float sLo2 = ((c[b2] - radius * 1.0001f) - boxPad) - pad, sHi2 = ((c[b2] + radius * 1.0001f) + boxPad) + pad;
                const bool counts =
                    vr::planar_round_valid(pr, q[b1], q[b2], std::numeric_limits<float>::infinity(), sLo1, sHi1, sLo2, sHi2);
                float lo[3], hi3[3];
                lo[a] = ca - pad, hi3[a] = ca + pad;
                lo[b1] = q[b1] - pad, hi3[b1] = q[b1] + pad;
                lo[b2] = q[b2] - pad, hi3[b2] = q[b2] + pad;
                bool ball = true;
                for (int j = 0; j < 3; ++j)
                  ball = ball && c[j] - radius <= hi3[j] && c[j] + radius >= lo[j];
                if (!counts || !ball) {
                  if (failed < 10)
                    std::printf("  (2) axis %d: q (%.9g %.9g %.9g) c (%.9g %.9g %.9g) r %.9g pad %.9g: counts %d ball %d\n", a, q[0], q[1], q[2],
                                c[0], c[1], c[2], radius, pad, (int)counts, (int)ball);
                  ++failed;
                }
                ++boxChecks;
                edgeAccepts += edge;
              }
            }
          }
  std::printf("%llu cases: %llu hit accepts, %llu neighbour accepts, %llu with t near tnear; %llu box checks, %llu of them at the acceptance edge\n",
              cases, hitAccepts, localAccepts, nearTnear, boxChecks, edgeAccepts);

  // ---- (3) the wall rule ------------------------------------------------------------------------------------------
  unsigned long long wallFree = 0, freeHits = 0, onWall = 0, outside = 0, onEdge = 0, emptyRects = 0, refusedOutside = 0;
  double minRatio = 1e300;
  for (int k = 0; k < WALL_CASES; ++k) {
    // the walls' rectangle: extents from 1 to 1000, offsets up to 2000 extents (the rule holds up to 1000)
    vr::PlanarWallRect w, in;
    const float e1 = 1.f + 999.f * g.unit() * g.unit(), e2 = 1.f + 999.f * g.unit() * g.unit();
    const float off1 = (g.u32() % 4u == 0u) ? -0.5f * e1 : g.sym(2000.f) * e1;
    const float off2 = (g.u32() % 4u == 0u) ? -0.5f * e2 : g.sym(2000.f) * e2;
    w.lo1 = off1, w.hi1 = off1 + e1, w.lo2 = off2, w.hi2 = off2 + e2;
    vr::planar_wall_inner(w.lo1, w.hi1, in.lo1, in.hi1);
    vr::planar_wall_inner(w.lo2, w.hi2, in.lo2, in.hi2);
    const float lo[2] = {w.lo1, w.lo2}, hi[2] = {w.hi1, w.hi2}, ilo[2] = {in.lo1, in.lo2}, ihi[2] = {in.hi1, in.hi2};
    bool empty = false;
    for (int j = 0; j < 2; ++j) {
      const float e = hi[j] - lo[j], C = std::fmax(std::fabs(lo[j]), std::fabs(hi[j]));
      if (!(C <= 1000.f * e)) {
        if (ilo[j] <= ihi[j]) {
          std::printf("  (3) [%.9g, %.9g]: beyond the rule's limit, yet the shrunk interval is not empty\n", lo[j], hi[j]);
          ++failed;
        }
        empty = true;
      }
    }
    emptyRects += empty;
    // the ray: plane z = ca with the normal (0, 0, 1), wall axes x and y
    const float ca = heights[g.u32() % 4u], s = 1.f, radius = 1.f, thresh = vr::uniform_disk_threshold(radius);
    float o[3], tq[2];
    const uint32_t kk = g.u32() % 8u;
    for (int j = 0; j < 2; ++j) {
      const uint32_t ko = g.u32() % 8u;
      o[j] = lo[j] + (hi[j] - lo[j]) * g.unit();
      if (ko == 0u)
        o[j] = lo[j];
      else if (ko == 1u)
        o[j] = hi[j];
      else if (ko == 2u)
        o[j] = down(lo[j]);
      else if (ko == 3u)
        o[j] = up(hi[j]);
      onWall += ko <= 1u;
      outside += ko == 2u || ko == 3u;
      // where the ray is aimed: anywhere around the rectangle, or at the shrunk rectangle's edge
      const float ea = empty ? lo[j] : ilo[j], eb = empty ? hi[j] : ihi[j];
      const uint32_t kq = g.u32() % 8u;
      tq[j] = lo[j] + (hi[j] - lo[j]) * (1.2f * g.unit() - 0.1f);
      if (kq == 0u)
        tq[j] = ea;
      else if (kq == 1u)
        tq[j] = eb;
      else if (kq == 2u)
        tq[j] = up(ea);
      else if (kq == 3u)
        tq[j] = down(eb);
      onEdge += kq <= 3u;
    }
    o[2] = ca + (kk == 0u ? 1e-4f * (1.f + g.sym(1e-6f)) : 0.01f + 30.f * g.unit()); // (kk == 0: t near tnear with d.z = -1)
    float d[3];
    d[2] = kk == 0u ? -1.f : -(0.02f + g.unit());
    const float tAim = (ca - o[2]) / d[2];
    d[0] = (tq[0] - o[0]) / tAim;
    d[1] = (tq[1] - o[1]) / tAim;
    if (kk == 1u) // a zero of either sign across: the ray runs along a wall's normal plane
      d[g.u32() & 1u] = (g.u32() & 1u) ? 0.f : -0.f;
    const vr::PlanarRound pr = vr::planar_round_point(true, o[0], o[1], o[2], d[0], d[1], d[2], o[2], d[2] * s, tnear, ca, s, radius, thresh);
    const bool isFree = vr::planar_wall_free(o[0], o[1], pr.qx, pr.qy, w, in);
    if (isFree && empty) {
      std::printf("  (3) a wall-free lane on a rectangle beyond the rule's limit\n");
      ++failed;
    }
    const bool out = o[0] < w.lo1 || o[0] > w.hi1 || o[1] < w.lo2 || o[1] > w.hi2;
    if (isFree && out) {
      std::printf("  (3) a wall-free lane with its origin outside the walls: o (%.9g %.9g)\n", o[0], o[1]);
      ++failed;
    }
    refusedOutside += out;
    wallFree += isFree;
    if (!isFree || !(pr.hitThr > 0.f))
      continue;
    ++freeHits;
    const float tLimit = pr.t * 1.001f; // (hit_walls_from, with the plane hit as the closest so far)
    for (int pair = 0; pair < 4; ++pair) {
      const int j = pair >> 1;
      const float W = (pair & 1) ? hi[j] : lo[j], oa = o[j], da = d[j];
      const float r0 = 1.0f / da;
      const float rcps[3] = {r0, up(r0), down(r0)};
      for (float rcp : rcps)
        if (wall_passes(W, oa, da, rcp, tLimit)) {
          if (failed < 10)
            std::printf("  (3) wall %d at %.9g passes the pre-test: o %.9g d %.9g t %.9g rcp %.9g, rectangle [%.9g, %.9g] shrunk [%.9g, %.9g] q %.9g\n",
                        pair, W, oa, da, pr.t, rcp, lo[j], hi[j], ilo[j], ihi[j], j ? pr.qy : pr.qx);
          ++failed;
        }
      const double c = (double)W - (double)oa;
      if ((c > 0. && da > 0.f) || (c < 0. && da < 0.f)) {
        const double ratio = c / (double)da / (double)pr.t;
        minRatio = std::fmin(minRatio, ratio);
        if (!(ratio >= 1.0017)) {
          if (failed < 10)
            std::printf("  (3) wall %d at %.9g: its parameter is %.9g t\n", pair, W, ratio);
          ++failed;
        }
      }
    }
  }
  std::printf("%d wall cases: %llu wall-free, %llu of them with a plane hit, %llu origins on a wall, %llu one ulp outside, %llu aims at the shrunk edge, "
              "%llu rectangles beyond the limit, %llu origins outside; smallest wall parameter %.6f t\n",
              WALL_CASES, wallFree, freeHits, onWall, outside, onEdge, emptyRects, refusedOutside, minRatio);
  std::printf("%llu failed checks\n", failed);
  return failed ? 1 : 0;
}
