// vr_gather.hpp — the arithmetic of gatherFlux (vr_gather.hip: gather_samples_kernel) in plain C++: the host compiler takes
// this file alone (tests/aux/gather.cpp), the kernel includes it.  What a sample IS lives here — the chunk's engine seed,
// the direction from (r1, r2, normal, mode, D), the outcome -> weight rule, the constants g_D(n), the quantisation q() and
// the final division, the quantised square q2() and the standard error of the adaptive gather (tests/aux/
// gather_adaptive.cpp) — so that the host program and the device compute the same bits from the same text: sincosf / powf
// are vr_libm.hpp's on both sides, every other operation is a single IEEE float or double operation in a fixed order
// (-ffp-contract=off).  include/viennaray_amd.h has the definition this implements.
#pragma once
#include <cmath>
#include <cstdint>

#include "vr_libm.hpp"

#if defined(__HIPCC__)
#define VR_GATHER_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define VR_GATHER_FN inline
#endif

namespace vr {

constexpr uint32_t GATHER_NORMAL = 0;         // VR_GATHER_NORMAL: the cosine law about the primitive's normal
constexpr uint32_t GATHER_SOURCE = 1;         // VR_GATHER_SOURCE: the source's own power-cosine law about u
constexpr uint32_t GATHER_SEED_XOR = 0x47415448u; // "GATH": S = rng seed ^ this
constexpr uint32_t GATHER_CHUNK = 64;         // samples per engine
constexpr int GATHER_FRAC_BITS = 40;          // VR_FLUX_FRAC_BITS
constexpr uint32_t GATHER_MAX_SUBS = 16;      // a chunk is walked as at most this many work items (a power of two)

struct GVec {
  float x, y, z;
};

// tea<3> (vr_rng.hpp: tea3, the tracer's seed hash)
VR_GATHER_FN uint32_t gather_tea3(uint32_t v0, uint32_t v1) {
  uint32_t s0 = 0;
  for (int n = 0; n < 3; ++n) {
    s0 += 0x9e3779b9u;
    v0 += ((v1 << 4) + 0xa341316cu) ^ (v1 + s0) ^ ((v1 >> 5) + 0xc8013ea4u);
    v1 += ((v0 << 4) + 0xad90777du) ^ (v0 + s0) ^ ((v0 >> 5) + 0x7e95761eu);
  }
  return v0;
}
// the std::mt19937_64 seed of chunk `chunk` of ORIGINAL primitive `prim`; rngSeed: the context's (vr_set_rng_seed)
VR_GATHER_FN uint32_t gather_chunk_seed(uint32_t prim, uint32_t rngSeed, uint32_t chunk) {
  return gather_tea3(prim, (rngSeed ^ GATHER_SEED_XOR) + chunk);
}
// libstdc++'s uniform float from one 64-bit engine output (vr_rng.hpp: canon_f32)
VR_GATHER_FN float gather_canon(uint64_t v) {
  const float f = (float)v * 5.42101086242752217e-20f; // 2^-64
  return f >= 1.0f ? 0.99999994f : f;
}

VR_GATHER_FN float gather_dot(const GVec &a, const GVec &b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; } // (vdot)
VR_GATHER_FN void gather_normalize(GVec &a) { // (vnormalize)
  const float n = sqrtf(gather_dot(a, a));
  if (n <= 0.f)
    return;
  a.x /= n;
  a.y /= n;
  a.z /= n;
}
VR_GATHER_FN float gather_axis(const GVec &v, int a) { return a == 0 ? v.x : (a == 1 ? v.y : v.z); }
VR_GATHER_FN void gather_set_axis(GVec &v, int a, float f) {
  v.x = a == 0 ? f : v.x;
  v.y = a == 1 ? f : v.y;
  v.z = a == 2 ? f : v.z;
}

// the centroid of a packed triangle record {v0, e1 = v0 - v1, e2 = v2 - v0}: (v0 + v1 + v2) / 3, each vertex rebuilt from
// the record
VR_GATHER_FN GVec gather_tri_centroid(const GVec &v0, const GVec &e1, const GVec &e2) {
  return GVec{((v0.x + (v0.x - e1.x)) + (v0.x + e2.x)) / 3.f, ((v0.y + (v0.y - e1.y)) + (v0.y + e2.y)) / 3.f,
              ((v0.z + (v0.z - e1.z)) + (v0.z + e2.z)) / 3.f};
}

// the frame of the source: tracing axis, the two axes of the source plane, and uSign = -posNeg: the sign along the tracing
// axis of u, the unit vector from the surface TO the source plane
struct GatherFrame {
  int rayDir, firstDir, secondDir;
  float uSign;
};

// VR_GATHER_NORMAL, D = 3: the cosine law about m (surface_sample, vr_generate.hpp: cosT = sqrtf(r2), Frisvad basis)
VR_GATHER_FN GVec gather_dir_normal3(float r1, float r2, const GVec &n) {
  const float cosT = sqrtf(r2), sinT = sqrtf(fmaxf(0.f, 1.f - cosT * cosT));
  float sinP, cosP;
  glibc_sincosf((float)(3.14159265358979323846 * 2.f * (double)r1), sinP, cosP);
  const float s = copysignf(1.f, n.z), a = -1.f / (s + n.z), b = n.x * n.y * a;
  const GVec t{1.f + s * n.x * n.x * a, s * b, -s * n.x}, b2{b, s + n.y * n.y * a, -n.y};
  const float ct = cosP * sinT, st = sinP * sinT;
  GVec d{(n.x * cosT + t.x * ct) + b2.x * st, (n.y * cosT + t.y * ct) + b2.y * st, (n.z * cosT + t.z * ct) + b2.z * st};
  gather_normalize(d);
  return d;
}
// VR_GATHER_NORMAL, D = 2: the in-plane cosine law about m (pdf cos(phi) / 2 over the half circle): sin(phi) = 2 r1 - 1,
// the tangent is m turned by +90 degrees in the plane; z = 0
VR_GATHER_FN GVec gather_dir_normal2(float r1, const GVec &n) {
  const float sinP = 2.f * r1 - 1.f, cosP = sqrtf(fmaxf(0.f, 1.f - sinP * sinP));
  GVec d{n.x * cosP - n.y * sinP, n.y * cosP + n.x * sinP, 0.f};
  gather_normalize(d);
  return d;
}
// VR_GATHER_SOURCE: the source's law about u — cosine_sample (vr_rng.hpp) with the tracer's exponent 1 / (n + 1) in the
// tracer's source frame (source_sample, vr_generate.hpp), the tracing-axis component towards the source; in 2-D followed
// by project_dir<2>
VR_GATHER_FN GVec gather_dir_source(float r1, float r2, float cosinePower, const GatherFrame &f, int D) {
  const float ee = 1.f / (cosinePower + 1.f);
  const float ang = (float)(3.14159265358979323846 * 2. * (double)r1);
  float sinP, cosP;
  glibc_sincosf(ang, sinP, cosP);
  const float cosT = glibc_powf(r2, ee);
  const float sinT = (float)sqrt(1. - (double)(cosT * cosT));
  GVec d{0.f, 0.f, 0.f};
  gather_set_axis(d, f.rayDir, f.uSign * cosT);
  gather_set_axis(d, f.firstDir, cosP * sinT);
  gather_set_axis(d, f.secondDir, sinP * sinT);
  if (D == 2 && d.z != 0.f) {
    d.z = 0.f;
    gather_normalize(d);
  }
  return d;
}
VR_GATHER_FN GVec gather_direction(uint32_t mode, int D, float r1, float r2, const GVec &normal, float cosinePower,
                                   const GatherFrame &f) {
  if (mode == GATHER_SOURCE)
    return gather_dir_source(r1, r2, cosinePower, f, D);
  return D == 2 ? gather_dir_normal2(r1, normal) : gather_dir_normal3(r1, r2, normal);
}
// c = u . omega of the initial direction
VR_GATHER_FN float gather_c(const GVec &dir, const GatherFrame &f) { return f.uSign * gather_axis(dir, f.rayDir); }

// how a sample ended
enum GatherEnd : int {
  GATHER_END_MISS = 0,    // left the scene without passing an IGNORE wall
  GATHER_END_IGNORED = 1, // left through an IGNORE wall
  GATHER_END_WALL = 2,    // stopped on a wall: the boundary-hit budget ran out
  GATHER_END_FRONT = 3,   // hit a primitive on its front side (direction . normal < 0)
  GATHER_END_BACK = 4     // hit a primitive on its back side
};

// c^e for 0 < c, e > 0 by vr_libm.hpp's powf, which handles neither subnormal arguments nor results below the doubles'
// range: a c below FLT_MIN counts as 0, and so does a power that is certainly below 2^-160 (an upper bound of log2(c) from
// the exponent field, and from log2(c) <= (c - 1) / ln 2) — a float 0 either way
VR_GATHER_FN float gather_pow(float c, float e) {
  if (c >= 1.f)
    return 1.f;
  if (!(c >= 1.17549435e-38f))
    return 0.f;
  const float expo = (float)((int)((vr_asuint(c) >> 23) & 0xffu) - 126); // log2(c) < expo
  if (e * expo < -160.f || e * (c - 1.f) * 1.44269502f < -160.f)
    return 0.f;
  return glibc_powf(c, e);
}

// The outcome -> weight rule.  g: g_D(n); n: cosinePower; c: u . omega of the INITIAL direction; mDotW: m_i . omega of
// the initial direction; emission: emission[j] of the primitive hit (read only for GATHER_END_FRONT with a table)
VR_GATHER_FN float gather_weight(int end, uint32_t mode, float g, float n, float c, float mDotW, bool haveEmission,
                                 float emission) {
  if (end == GATHER_END_MISS && c > 0.f) {
    if (mode == GATHER_SOURCE)
      return mDotW > 0.f ? mDotW / c : 0.f;
    return n == 1.f ? g : g * gather_pow(c, n - 1.f);
  }
  if (end == GATHER_END_FRONT && haveEmission)
    return emission;
  return 0.f;
}

// The largest weight a sample of a call with `samples` samples may count: 2^22 / (samples rounded up to a power of two),
// so that samples x wmax x 2^40 <= 2^62 — neither a chunk's sum in registers nor a primitive's int64 sum can overflow,
// whatever the emission table holds.  4096 samples: 1024.  (The entry points refuse a call whose NORMAL weights, at most
// g_D(n), would be cut: samples x g < 2^22.)
VR_GATHER_FN float gather_wmax(uint32_t samples) {
  float w = 4194304.f; // 2^22
  for (uint64_t p = 1; p < (uint64_t)samples; p *= 2)
    w *= 0.5f;
  return w;
}
// q(w): the flux accumulators' quantisation (vr_trace_kernel.hpp: weight_fx).  A weight that is not positive (NaN
// included) counts 0, one above wmax counts wmax
VR_GATHER_FN int64_t gather_q(float w, float wmax) {
  if (!(w > 0.f))
    return 0;
  const float wc = w > wmax ? wmax : w;
  return (int64_t)((double)wc * 1099511627776.0 + 0.5);
}
// out[i] from the int64 sum of K samples
VR_GATHER_FN float gather_result(int64_t sum, uint32_t samples) {
  return (float)((double)sum / 1099511627776.0 / (double)samples);
}

// ---- the second sum and the standard error (vr_gather_sums*, vr_gather_adaptive*) ------------------------------------
constexpr int GATHER_SQ_FRAC_BITS = 28;   // the fixed point of a squared weight
constexpr int GATHER_SQ_CUT_LOG2 = 11;    // a squared weight is that of min(w, wmax, 2^11)
// q2(w): the quantised SQUARE of the weight q() counts.  0 for a weight that is not positive (NaN included); otherwise
// wc = min(w, wmax, 2048) and (int64)(wc * wc * 2^28 + 0.5) — the product of two floats is exact in double.
// The sum of `budget` such terms stays within 2^61 for every budget the gather accepts (samples x g <= 2^22, g >= 1):
//   budget <= 2^11:  wc <= 2^11, a term <= 2^(22 + 28) = 2^50, the sum <= 2^11 x 2^50 = 2^61;
//   budget  = 2^b > 2^11:  wc <= wmax = 2^(22 - b), a term <= 2^(72 - 2b), the sum <= 2^(72 - b) < 2^61.
// (tests/aux/gather_adaptive.cpp walks every power-of-two budget.)
static_assert(GATHER_SQ_CUT_LOG2 + 2 * GATHER_SQ_CUT_LOG2 + GATHER_SQ_FRAC_BITS == 61 &&
                  2 * 22 + GATHER_SQ_FRAC_BITS - (GATHER_SQ_CUT_LOG2 + 1) < 61,
              "a primitive's int64 sum of squares cannot overflow");
VR_GATHER_FN int64_t gather_q2(float w, float wmax) {
  if (!(w > 0.f))
    return 0;
  float wc = w > wmax ? wmax : w;
  wc = wc > 2048.f ? 2048.f : wc;
  return (int64_t)((double)wc * (double)wc * 268435456.0 + 0.5);
}
// The mean m1 and the squared standard error se2 of the mean of K samples (K >= 2; the gather's K is >= 64) from the two
// exact sums S1 = sum q(w), S2 = sum q2(w):
//   m1 = (double)S1 * 2^-40 / K;  m2 = (double)S2 * 2^-28 / K;  v = m2 - m1 * m1, 0 unless v > 0;  se2 = v / (K - 1).
// Every operation is one IEEE double operation in this order, contraction off, so that the host, the device and numpy
// float64 agree bit for bit
#if defined(__clang__)
#define VR_GATHER_NO_CONTRACT _Pragma("clang fp contract(off)")
#define VR_GATHER_NO_CONTRACT_ATTR
#elif defined(__GNUC__)
#define VR_GATHER_NO_CONTRACT
#define VR_GATHER_NO_CONTRACT_ATTR __attribute__((optimize("fp-contract=off")))
#else
#define VR_GATHER_NO_CONTRACT
#define VR_GATHER_NO_CONTRACT_ATTR
#endif
VR_GATHER_NO_CONTRACT_ATTR VR_GATHER_FN void gather_moments(int64_t S1, int64_t S2, uint32_t K, double &m1, double &se2) {
  VR_GATHER_NO_CONTRACT
  const double k = (double)K;
  m1 = (double)S1 * 9.094947017729282379150390625e-13 / k; // 2^-40
  const double m2 = (double)S2 * 3.7252902984619140625e-09 / k; // 2^-28
  const double sq = m1 * m1;
  double v = m2 - sq;
  if (!(v > 0.))
    v = 0.;
  se2 = v / (k - 1.);
}
VR_GATHER_FN double gather_stderr2(int64_t S1, int64_t S2, uint32_t K) {
  double m1, se2;
  gather_moments(S1, S2, K, m1, se2);
  return se2;
}
// The stopping rule of a primitive after K samples: tol = max(rel * m1, abs), converged if and only if se2 <= tol * tol.
// rel == abs == 0 means "never": every primitive runs to maxSamples, one of zero variance included.  A primitive whose
// samples so far all weigh 0 has m1 = se2 = 0 and is converged at minSamples under any positive target: the call cannot
// know better — nothing it has seen tells a primitive in full shadow from one whose first bright sample is still to come
VR_GATHER_NO_CONTRACT_ATTR VR_GATHER_FN bool gather_converged(int64_t S1, int64_t S2, uint32_t K, float rel, float abs) {
  VR_GATHER_NO_CONTRACT
  if (!(rel > 0.f) && !(abs > 0.f))
    return false;
  double m1, se2;
  gather_moments(S1, S2, K, m1, se2);
  const double r = (double)rel * m1, a = (double)abs;
  const double tol = r > a ? r : a;
  return se2 <= tol * tol;
}

// ---- gatherPaths (vr_gather_paths*): a sample followed through its reflections ---------------------------------------
constexpr uint32_t GATHER_REFLECT_SPECULAR = 0;        // VR_GATHER_REFLECT_SPECULAR: the mirror direction at every vertex
constexpr uint32_t GATHER_REFLECT_DIFFUSE = 1;         // VR_GATHER_REFLECT_DIFFUSE: the cosine law about the normal hit
constexpr uint32_t GATHER_PATH_SEED_XOR = 0x50415448u; // "PATH": the counter draws' key starts from rng seed ^ this
constexpr uint32_t GATHER_MAX_BOUNCES = 65535;         // VR_GATHER_MAX_BOUNCES
// the two ends a path adds to a sample's (both weigh 0)
constexpr int GATHER_END_BOUNCES = 5;  // a front-side hit with maxBounces bounces made
constexpr int GATHER_END_ABSORBED = 6; // a front-side hit that took the throughput to 0

// tea<8>: gather_tea3's rounds, eight of them — every output bit depends on every input bit, which a counter needs
VR_GATHER_FN uint32_t gather_tea8(uint32_t v0, uint32_t v1) {
  uint32_t s0 = 0;
  for (int n = 0; n < 8; ++n) {
    s0 += 0x9e3779b9u;
    v0 += ((v1 << 4) + 0xa341316cu) ^ (v1 + s0) ^ ((v1 >> 5) + 0xc8013ea4u);
    v1 += ((v0 << 4) + 0xad90777du) ^ (v0 + s0) ^ ((v0 >> 5) + 0x7e95761eu);
  }
  return v0;
}
// The counter draw of a DIFFUSE vertex: a pure function of (rng seed, ORIGINAL id of the primitive the path starts from,
// sample index, bounce index) — no engine, nothing of chunks, ranges or earlier samples.  key: one hash per path
VR_GATHER_FN uint32_t gather_path_key(uint32_t rngSeed, uint32_t prim, uint32_t sample) {
  return gather_tea8(prim, (rngSeed ^ GATHER_PATH_SEED_XOR) + sample);
}
// uniform `which` (0: r1, 1: r2) of bounce `bounce`: the top 24 bits of a hash, in [0, 1) (both operations are exact)
VR_GATHER_FN float gather_path_uniform(uint32_t key, uint32_t bounce, uint32_t which) {
  return (float)(gather_tea8(key, 2u * bounce + which) >> 8) * 5.9604644775390625e-08f; // 2^-24
}
VR_GATHER_FN void gather_path_draw(uint32_t rngSeed, uint32_t prim, uint32_t sample, uint32_t bounce, float &r1, float &r2) {
  const uint32_t key = gather_path_key(rngSeed, prim, sample);
  r1 = gather_path_uniform(key, bounce, 0u);
  r2 = gather_path_uniform(key, bounce, 1u);
}
// the direction a DIFFUSE vertex leaves along: the cosine law about the normal hit, from the counter draw
VR_GATHER_FN GVec gather_path_diffuse(int D, uint32_t rngSeed, uint32_t prim, uint32_t sample, uint32_t bounce, const GVec &n) {
  float r1, r2;
  gather_path_draw(rngSeed, prim, sample, bounce, r1, r2);
  return D == 2 ? gather_dir_normal2(r1, n) : gather_dir_normal3(r1, r2, n);
}
// T after a front-side hit of a primitive of reflectivity rho: one float32 multiply
VR_GATHER_FN float gather_path_throughput(float T, float rho) { return T * rho; }
// The end -> weight rule of a path.  cEnd: u . omega of the FINAL direction; T: the product of the reflectivities on the
// way.  gather_weight's NORMAL rule on cEnd, then one multiply by T; every end but the source weighs 0
VR_GATHER_FN float gather_path_weight(int end, float g, float n, float cEnd, float T) {
  if (end != GATHER_END_MISS)
    return 0.f;
  return gather_weight(end, GATHER_NORMAL, g, n, cEnd, 0.f, false, 0.f) * T;
}
// a reflectivity the entry points accept (vr_radiosity.hpp: radiosity_rho_ok has the same rule)
VR_GATHER_FN bool gather_path_rho_ok(float rho) { return rho >= 0.f && rho <= 1.f; }

// ---- gatherAngular (vr_gather_angular*): a path weighed by tabulated angular laws -------------------------------------
constexpr uint32_t GATHER_LAW_MIN = 2, GATHER_LAW_MAX = 256; // entries of a law
// the three laws' places in the device table (GATHER_LAW_MAX floats each) and in GatherArgs::lawCount
constexpr int GATHER_LAW_SOURCE = 0, GATHER_LAW_REFLECTIVITY = 1, GATHER_LAW_YIELD = 2;
// An angular law: M float32 values read as the piecewise-linear function of a cosine x in [0, 1] with nodes at
// x_k = k / (M - 1).  float32, one IEEE operation per step in this order, contraction off, so that the host, the device and
// numpy float32 agree bit for bit.  A NaN x reads as 0 (fmaxf returns its other argument)
VR_GATHER_NO_CONTRACT_ATTR VR_GATHER_FN float gather_law(const float *t, uint32_t M, float x) {
  VR_GATHER_NO_CONTRACT
  const float xc = fminf(fmaxf(x, 0.f), 1.f);
  const float xs = xc * (float)(M - 1u);
  int k = (int)xs;
  k = k < (int)M - 2 ? k : (int)M - 2;
  const float f = xs - (float)k;
  const float d = t[k + 1] - t[k];
  const float fd = f * d;
  return t[k] + fd;
}
// what an entry of each law may be: finite and >= 0 (source, yield), in [0, 1] (reflectivity)
VR_GATHER_FN bool gather_law_entry_ok(int which, float v) {
  if (which == GATHER_LAW_REFLECTIVITY)
    return v >= 0.f && v <= 1.f;
  return v >= 0.f && v <= 3.40282347e+38f;
}
VR_GATHER_FN bool gather_law_count_ok(uint32_t M) { return M >= GATHER_LAW_MIN && M <= GATHER_LAW_MAX; }
// the lowest index whose entry is refused, M where there is none
inline uint32_t gather_law_first_bad(int which, const float *t, uint32_t M) {
  for (uint32_t k = 0; k < M; ++k)
    if (!gather_law_entry_ok(which, t[k]))
      return k;
  return M;
}
inline float gather_law_max(const float *t, uint32_t M) {
  float m = t[0];
  for (uint32_t k = 1; k < M; ++k)
    m = t[k] > m ? t[k] : m;
  return m;
}
// Z of a source law L (a host function, double): the forward source has the direction density L(c) c / Z per solid angle.
// The interpolant integrated exactly, segment by segment, L = a + b c on [c0, c1]:
//   D = 3: Z = 2 pi int_0^1 L(c) c dc,                  antiderivative a c^2 / 2 + b c^3 / 3;
//   D = 2: Z = 2 int_0^1 L(c) c / sqrt(1 - c^2) dc,     antiderivative -a s + b (asin(c) - c s) / 2, s = sqrt(1 - c^2).
inline double gather_law_norm(const float *t, uint32_t M, int D) {
  const double h = 1. / (double)(M - 1u);
  double sum = 0.;
  for (uint32_t k = 0; k + 1u < M; ++k) {
    const double c0 = (double)k * h, c1 = k + 2u == M ? 1. : (double)(k + 1u) * h;
    const double b = ((double)t[k + 1] - (double)t[k]) / (c1 - c0), a = (double)t[k] - b * c0;
    if (D == 3) {
      sum += a * (c1 - c0) * (c1 + c0) / 2. + b * (c1 - c0) * (c1 * c1 + c1 * c0 + c0 * c0) / 3.;
    } else {
      const double s0 = std::sqrt((1. - c0) * (1. + c0)), s1 = std::sqrt((1. - c1) * (1. + c1));
      sum += a * (s0 - s1) + b * ((std::asin(c1) - c1 * s1) - (std::asin(c0) - c0 * s0)) / 2.;
    }
  }
  return D == 3 ? 2. * 3.14159265358979323846 * sum : 2. * sum;
}
// g_L: the weight of a path that reaches the source is g_L L(c_end) T — the ratio of the source's law L(c) c / Z and the
// receiver's cosine law c / pi (3-D), c / 2 (2-D).  L = 1 gives exactly 1: Z is pi (2) to a few ulps of a double
inline float gather_law_g(const float *t, uint32_t M, int D) {
  return (float)((D == 3 ? 3.14159265358979323846 : 2.) / gather_law_norm(t, M, D));
}
// The end -> weight rule of a path with laws (a law that is nullptr is absent): gather_path_weight's, with
// g_L L(c_end) in place of g c_end^(n - 1) where there is a source law, and one more multiply, last, by the yield at
// mu0 = m_i . omega_0 of the INITIAL direction:  w = ((g_L L(c_end) or g c_end^(n - 1)) * T) * Y(mu0)
VR_GATHER_NO_CONTRACT_ATTR VR_GATHER_FN float gather_path_weight_laws(int end, float g, float n, float cEnd, float T, const float *L,
                                                                      uint32_t ML, float gL, const float *Y, uint32_t MY,
                                                                      float mu0) {
  VR_GATHER_NO_CONTRACT
  if (end != GATHER_END_MISS)
    return 0.f;
  float w;
  if (L) {
    if (!(cEnd > 0.f))
      return 0.f;
    const float s = gL * gather_law(L, ML, cEnd);
    w = s * T;
  } else {
    w = gather_weight(end, GATHER_NORMAL, g, n, cEnd, 0.f, false, 0.f) * T;
  }
  if (Y)
    w = w * gather_law(Y, MY, mu0);
  return w;
}
// T after a front-side hit with a reflectivity law R at mu = n_j . (the direction the path leaves along): two multiplies
VR_GATHER_NO_CONTRACT_ATTR VR_GATHER_FN float gather_path_throughput_law(float Trho, const float *R, uint32_t MR, float mu) {
  VR_GATHER_NO_CONTRACT
  return Trho * gather_law(R, MR, mu);
}

// ---- gatherSpecies (vr_gather_species*): several species weighed along one traced path -------------------------------
constexpr uint32_t GATHER_MAX_SPECIES = 4; // VR_GATHER_MAX_SPECIES
#if defined(__clang__)
#define VR_GATHER_UNROLL _Pragma("unroll")
#else
#define VR_GATHER_UNROLL
#endif
// The step of NS species at a front-side hit of the path they share, in two halves: the leaving direction — and with it
// mu — is formed between them, once, and only if a species is left to follow it.  alive: bit s set while species s still
// follows the path; a species whose T reaches 0 leaves the mask and its T is not touched again (it weighs 0, it is not
// weighed).  Each species' multiplies are gather_path_throughput and gather_path_throughput_law, in that order: the T and
// the vertex of death of species s are those of the single-species path with its rho and R.
// First half: T_s <- T_s * rho_s of the primitive hit.  Returns the species still alive; 0: the path ends there
template <int NS> VR_GATHER_FN unsigned gather_species_absorb(float (&T)[NS], unsigned alive, const float (&rho)[NS]) {
  VR_GATHER_UNROLL
  for (int s = 0; s < NS; ++s)
    if ((alive >> s) & 1u) {
      T[s] = gather_path_throughput(T[s], rho[s]);
      if (T[s] == 0.f)
        alive &= ~(1u << s);
    }
  return alive;
}
// Second half: T_s <- T_s * R_s(mu) for the living species that have a reflectivity law (MR[s] != 0: R[s] holds it), mu =
// n_j . (the direction the path leaves along)
template <int NS>
VR_GATHER_FN unsigned gather_species_reflect(float (&T)[NS], unsigned alive, const float *const (&R)[NS], const uint32_t (&MR)[NS],
                                             float mu) {
  VR_GATHER_UNROLL
  for (int s = 0; s < NS; ++s)
    if (((alive >> s) & 1u) && MR[s]) {
      T[s] = gather_path_throughput_law(T[s], R[s], MR[s], mu);
      if (T[s] == 0.f)
        alive &= ~(1u << s);
    }
  return alive;
}
// both halves for a mu that is known beforehand (a host program's view of the step; the kernel calls the halves)
template <int NS>
VR_GATHER_FN unsigned gather_species_step(float (&T)[NS], unsigned alive, const float (&rho)[NS], const float *const (&R)[NS],
                                          const uint32_t (&MR)[NS], float mu) {
  alive = gather_species_absorb<NS>(T, alive, rho);
  if (!alive)
    return 0u;
  return gather_species_reflect<NS>(T, alive, R, MR, mu);
}

// ---- gatherSpeciesAdaptive (vr_gather_species_adaptive*): every species of a primitive to its own target --------------
// One round's verdict of one primitive (gather_species_decide_kernel; tests/aux/gather_species_adaptive.cpp).  mask: the
// species still sampling there; S1[s], S2[s]: the two sums of species s after K samples — read for the species in the mask
// alone: one outside it stopped at an older K, its sums are not sums over K.  Each species in the mask is tested by
// gather_converged on its own sums under its own targets, which is the test its own adaptive call makes at this K.
// Returns the species that failed: the next round's mask, or with `last` (K == maxSamples) the unconverged.  writes: the
// species whose outputs are written at this K — those that converged, with `last` all of the mask
VR_GATHER_FN unsigned gather_species_decide(const int64_t *S1, const int64_t *S2, uint32_t numSpecies, uint32_t K, const float *rel,
                                            const float *abs, unsigned mask, bool last, unsigned &writes) {
  unsigned failed = 0u;
  VR_GATHER_UNROLL
  for (uint32_t s = 0; s < GATHER_MAX_SPECIES; ++s)
    if (s < numSpecies && ((mask >> s) & 1u) && !gather_converged(S1[s], S2[s], K, rel[s], abs[s]))
      failed |= 1u << s;
  writes = last ? mask : mask & ~failed;
  return failed;
}

// ---- gatherEnergy (vr_gather_energy*): an ion's energy carried along a path ------------------------------------------
constexpr uint32_t GATHER_ENERGY_COUNTER = 0x454E5247u; // "ENRG": the counter of the energy draw (the bounce draws' stop at 131071)
constexpr int GATHER_END_ENERGY = 7;                    // VR_GATHER_END_ENERGY: the arrival energy has entered the yield's zero region
// the three energy tables' places in the device table (GATHER_LAW_MAX floats each) and in GatherEnergyArgs::count
constexpr int GATHER_ENERGY_YIELD = 0, GATHER_ENERGY_QUANTILES = 1, GATHER_ENERGY_RETENTION = 2;
// u of a path: the top 24 bits of one hash of the path's key (gather_path_key), in [0, 1); both operations are exact
VR_GATHER_FN float gather_energy_u(uint32_t key) {
  return (float)(gather_tea8(key, GATHER_ENERGY_COUNTER) >> 8) * 5.9604644775390625e-08f; // 2^-24
}
// E0: the source's inverse CDF Q read at u, or (Q == nullptr) the one energy of a monoenergetic source
VR_GATHER_FN float gather_energy_source(const float *Q, uint32_t MQ, float u, float sourceEnergy) {
  return Q ? gather_law(Q, MQ, u) : sourceEnergy;
}
// P after a front-side hit the path goes on from: one multiply by the retention law at mu, the reflectivity law's mu
VR_GATHER_NO_CONTRACT_ATTR VR_GATHER_FN float gather_energy_retain(float P, const float *eps, uint32_t Meps, float mu) {
  VR_GATHER_NO_CONTRACT
  return P * gather_law(eps, Meps, mu);
}
// e: the arrival energy in the yield table's units — the product first, then the division
VR_GATHER_NO_CONTRACT_ATTR VR_GATHER_FN float gather_energy_arrival(float E0, float P, float energyMax) {
  VR_GATHER_NO_CONTRACT
  const float EP = E0 * P;
  return EP / energyMax;
}
// the last multiply of a path's weight: by the energy yield at e
VR_GATHER_NO_CONTRACT_ATTR VR_GATHER_FN float gather_energy_weight(float wAngular, const float *YE, uint32_t MY, float e) {
  VR_GATHER_NO_CONTRACT
  return wAngular * gather_law(YE, MY, e);
}
// Z0: the leading entries of an energy yield that are 0
inline uint32_t gather_energy_zeros(const float *YE, uint32_t MY) {
  uint32_t z = 0;
  while (z < MY && YE[z] == 0.f)
    ++z;
  return z;
}
// The cut (Z0 >= 2): true when e lies where the yield reads exactly 0 — xs, gather_law's own, is below node Z0 - 1, so the
// look-up interpolates between two entries that are both 0.  e = (E0 P) / energyMax never rises along a path: P only takes
// multiplies by values in [0, 1] and every rounding is monotone, so a path for which this holds weighs 0 whatever follows
VR_GATHER_NO_CONTRACT_ATTR VR_GATHER_FN bool gather_energy_cut(float e, uint32_t MY, uint32_t Z0) {
  VR_GATHER_NO_CONTRACT
  const float xc = fminf(fmaxf(e, 0.f), 1.f);
  const float xs = xc * (float)(MY - 1u);
  return xs < (float)(Z0 - 1u);
}
// what an entry of each energy table may be: finite and >= 0 (yield, quantiles), in [0, 1] (retention)
VR_GATHER_FN bool gather_energy_entry_ok(int which, float v) {
  return gather_law_entry_ok(which == GATHER_ENERGY_RETENTION ? GATHER_LAW_REFLECTIVITY : GATHER_LAW_YIELD, v);
}

// g_D(n) (a host function; the kernel takes the float): g_3 = (n + 1) / 2, g_2 = 2 / C_n with
// C_n = sqrt(pi) Gamma((n + 1) / 2) / Gamma(n / 2 + 1) — the weight of a sample that reaches the source is the ratio of
// the source's normalised law (n + 1) / (2 pi) c^n (3-D), c^n / C_n (2-D) and the receiver's cosine law c / pi, c / 2 for
// a receiver facing the source; n == 1 gives exactly 1
inline float gather_g(float n, int D) {
  if (n == 1.f)
    return 1.f;
  if (D == 3)
    return (n + 1.f) * 0.5f;
  const double cn = std::sqrt(3.14159265358979323846) * std::exp(std::lgamma(((double)n + 1.) / 2.) - std::lgamma((double)n / 2. + 1.));
  return (float)(2. / cn);
}

} // namespace vr
