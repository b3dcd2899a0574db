// The planar-disk candidate tests (viennaray_amd/csrc/vr_planar_disks.hpp) on the host against the forms they stand for:
// hit_disc_uniform and local_disc_hit_uniform (vr_intersect.hpp), restated below in plain float.  Compiled with
// -ffp-contract=off -fno-fast-math like the library: the same operations in the same order as on the device.
//
// Configurations: plane heights +0, -0, 0.3f, -7.25f  x  s = +1, -1  x  the axis x, y, z  x  the four sign patterns of the
// normal's two zeros: 96, with CASES_PER_CONFIG random cases each (more than 10^7 in all).  A case is a ray, a centre on
// the plane and a radius.  Mixed into every operand: +0, -0, denormals; origins exactly on the plane (a sixth of the
// cases); directions with a zero along the axis (divisor == 0) or a tiny one (|prod| < 1e-6); infinite and NaN origin
// components.  Half of the centres lie near the point where the ray crosses the plane, so that both tests accept often.
// Required: the same decision from both forms in every case, and the same bits of t wherever the hit test accepts; a
// lane that takes no part (on = false) is refused by both per-candidate forms.
// Then the host's axis rule on a table of normals.  Prints the counts and "N failed checks"; exit status 1 if N > 0.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>

#include "../../viennaray_amd/csrc/vr_planar_disks.hpp"
#include "../../viennaray_amd/csrc/vr_uniform_disks.hpp"

static const int CASES_PER_CONFIG = 110000;

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

// ---- the existing forms (vr_intersect.hpp), plain float -----------------------------------------------------------
static float edot(const float *a, const float *b) { return a[0] * b[0] + (a[1] * b[1] + a[2] * b[2]); }
static float vdot(const float *a, const float *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
static bool ref_hit(const float *o, const float *d, float tnear, const float *c, const float *n, float divisor, float radius,
                    float &tOut) {
  const float co[3] = {c[0] - o[0], c[1] - o[1], c[2] - o[2]};
  const float t = edot(co, n) / divisor;
  const float p[3] = {o[0] + d[0] * t - c[0], o[1] + d[1] * t - c[1], o[2] + d[2] * t - c[2]};
  const float dist2 = edot(p, p);
  tOut = t;
  return (divisor != 0.f) & (tnear <= t) & (t <= 3.402823466e+38f) & (dist2 < radius * radius);
}
static bool ref_local(const float *ro, const float *rd, const float *c, const float *n, float prod, float nro, float thresh) {
  const float ddneg = vdot(c, n);
  const float tt = (ddneg - nro) / prod;
  float hp[3] = {rd[0] * tt + ro[0], rd[1] * tt + ro[1], rd[2] * tt + ro[2]};
  hp[0] = hp[0] - c[0];
  hp[1] = hp[1] - c[1];
  hp[2] = hp[2] - c[2];
  return !(prod > 0.f) & !(std::fabs(prod) < 1e-6f) & !(tt <= 0.f) & (vdot(hp, hp) < thresh);
}

// ---- operands -----------------------------------------------------------------------------------------------------
struct Gen {
  std::mt19937_64 rng{20250117ull};
  uint32_t u32() { return (uint32_t)(rng() >> 32); }
  float unit() { return (float)(u32() >> 8) * (1.f / 16777216.f); } // [0, 1)
  float sym(float a) { return (2.f * unit() - 1.f) * a; }
  float denormal() { return from_bits((u32() & 0x807FFFFFu) | 1u); }
  // a finite coordinate: mostly ordinary, now and then a zero of either sign or a denormal
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

int main() {
  const float heights[4] = {0.f, -0.f, 0.3f, -7.25f};
  const float radii[3] = {0.8660254f, 0.43301272f, 1.0f};
  const float tnear = 1e-4f; // (vr_trace_kernel.hpp: the one value the kernel passes)
  Gen g;
  unsigned long long cases = 0, failed = 0, hitAccepts = 0, localAccepts = 0, onPlane = 0, zeroDiv = 0, tinyProd = 0, nonFinite = 0;
  for (int hi = 0; hi < 4; ++hi)
    for (int si = 0; si < 2; ++si)
      for (int a = 0; a < 3; ++a)
        for (int zp = 0; zp < 4; ++zp) {
          const float ca = heights[hi], s = si ? -1.f : 1.f;
          const int b1 = (a + 1) % 3, b2 = (a + 2) % 3;
          float n[3];
          n[a] = s;
          n[b1] = (zp & 1) ? -0.f : 0.f;
          n[b2] = (zp & 2) ? -0.f : 0.f;
          const uint32_t nw[3] = {to_bits(n[0]), to_bits(n[1]), to_bits(n[2])};
          if (vr::planar_disk_axis(nw) != a) {
            std::printf("  the axis rule refuses the normal (%g, %g, %g)\n", n[0], n[1], n[2]);
            ++failed;
          }
          for (int k = 0; k < CASES_PER_CONFIG; ++k) {
            float o[3], d[3], c[3];
            for (int j = 0; j < 3; ++j) {
              o[j] = g.coord(8.f);
              d[j] = g.coord(1.f);
            }
            // the origin along the axis: above or below the plane, a sixth of them exactly on it
            const uint32_t ko = g.u32() % 6u;
            if (ko == 0u) {
              o[a] = ca;
              ++onPlane;
            } else if (ko <= 3u) {
              o[a] = ca + s * (0.01f + 4.f * g.unit()); // (on the normal's side: where the source is)
            }
            // the direction along the axis: towards the plane mostly; a zero (divisor == 0) or a tiny one now and then
            const uint32_t kd = g.u32() % 16u;
            if (kd == 0u) {
              d[a] = (g.u32() & 1u) ? 0.f : -0.f;
              ++zeroDiv;
            } else if (kd == 1u) {
              d[a] = g.sym(2e-6f);
              ++tinyProd;
            } else if (kd == 2u) {
              d[a] = g.denormal();
              ++tinyProd;
            } else if (kd <= 10u) {
              d[a] = -s * (0.05f + g.unit());
            }
            if (g.u32() % 32u == 0u) { // an origin that is no point
              o[g.u32() % 3u] = g.nonfinite();
              ++nonFinite;
            }
            // the centre: on the plane; half of them near where the ray crosses it
            c[a] = ca;
            c[b1] = g.coord(8.f);
            c[b2] = g.coord(8.f);
            if (g.u32() & 1u) {
              const double t = ((double)ca - (double)o[a]) / (double)d[a];
              const double h1 = (double)o[b1] + (double)d[b1] * t, h2 = (double)o[b2] + (double)d[b2] * t;
              if (std::isfinite(h1) && std::isfinite(h2) && std::fabs(h1) < 1e6 && std::fabs(h2) < 1e6) {
                c[b1] = (float)h1 + g.sym(1.2f);
                c[b2] = (float)h2 + g.sym(1.2f);
              }
            }
            const float radius = radii[g.u32() % 3u], thresh = vr::uniform_disk_threshold(radius);
            // per ray and round: the caller's three dot products, as pq_hit_packet makes them
            const float divisor = edot(d, n), prod = vdot(n, d), nro = vdot(n, o);
            float tRef = 0.f;
            const bool hitRef = ref_hit(o, d, tnear, c, n, divisor, radius, tRef);
            const bool locRef = ref_local(o, d, c, n, prod, nro, thresh);
            const vr::PlanarHit ph = vr::planar_hit_round(true, o[0], o[1], o[2], d[0], d[1], d[2], o[a], tnear, ca, s, divisor);
            const vr::PlanarLocal pl = vr::planar_local_round(true, o[0], o[1], o[2], d[0], d[1], d[2], ca, s, prod, nro);
            const bool hitNew = vr::planar_hit_cand(ph, c[0], c[1], c[2], radius);
            const bool locNew = vr::planar_local_cand(pl, c[0], c[1], c[2], thresh);
            bool bad = hitNew != hitRef || locNew != locRef || (hitRef && to_bits(ph.t) != to_bits(tRef));
            if ((k & 15) == 0) { // a lane that takes no part
              const vr::PlanarHit ph0 = vr::planar_hit_round(false, o[0], o[1], o[2], d[0], d[1], d[2], o[a], tnear, ca, s, divisor);
              const vr::PlanarLocal pl0 = vr::planar_local_round(false, o[0], o[1], o[2], d[0], d[1], d[2], ca, s, prod, nro);
              bad = bad || vr::planar_hit_cand(ph0, c[0], c[1], c[2], radius) || vr::planar_local_cand(pl0, c[0], c[1], c[2], thresh);
            }
            if (bad) {
              if (failed < 10)
                std::printf("  ca %g s %g axis %d zeros %d: o (%.9g %.9g %.9g) d (%.9g %.9g %.9g) c (%.9g %.9g %.9g) r %.9g: hit %d/%d t %08x/%08x local %d/%d\n",
                            ca, s, a, zp, o[0], o[1], o[2], d[0], d[1], d[2], c[0], c[1], c[2], radius, (int)hitRef, (int)hitNew,
                            to_bits(tRef), to_bits(ph.t), (int)locRef, (int)locNew);
              ++failed;
            }
            hitAccepts += hitRef;
            localAccepts += locRef;
            ++cases;
          }
        }
  std::printf("%llu cases: %llu hit accepts, %llu neighbour accepts, %llu origins on the plane, %llu zero divisors, %llu tiny products, %llu non-finite origins\n",
              cases, hitAccepts, localAccepts, onPlane, zeroDiv, tinyProd, nonFinite);

  // ---- the host's axis rule --------------------------------------------------------------------------------------
  const float nan = std::numeric_limits<float>::quiet_NaN(), den = from_bits(1u) /* 1e-45 */;
  const struct {
    float n[3];
    int axis;
  } table[] = {{{0.f, 0.f, 1.f}, 2},         {{-0.f, 0.f, -1.f}, 2},  {{1.f, 0.f, 0.f}, 0},   {{0.f, -1.f, -0.f}, 1},
               {{0.f, 0.f, 0.99999994f}, -1}, {{den, 0.f, 1.f}, -1},   {{nan, 0.f, 1.f}, -1},  {{0.f, 0.f, nan}, -1},
               {{0.f, 0.f, 0.f}, -1},         {{1.f, 0.f, 1.f}, -1},   {{0.f, 0.f, 2.f}, -1},  {{0.f, 1.0000001f, 0.f}, -1}};
  unsigned rows = 0;
  for (const auto &row : table) {
    const uint32_t w[3] = {to_bits(row.n[0]), to_bits(row.n[1]), to_bits(row.n[2])};
    if (vr::planar_disk_axis(w) != row.axis) {
      std::printf("  axis rule: (%.9g, %.9g, %.9g) gives %d, expected %d\n", row.n[0], row.n[1], row.n[2], vr::planar_disk_axis(w), row.axis);
      ++failed;
    }
    ++rows;
  }
  std::printf("%u normals of the axis table\n%llu failed checks\n", rows, failed);
  return failed ? 1 : 0;
}
