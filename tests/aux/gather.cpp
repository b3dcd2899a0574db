// The arithmetic of gatherFlux (viennaray_amd/csrc/vr_gather.hpp) on the host: the header the kernel includes, taken by the
// host compiler alone.
//   gather                 the checks: the outcome -> weight table, q() and the final division, the power guard, and the
//                          directions of 10^5 samples per case from a std::mt19937_64 (unit length, hemisphere, means).
//                          Prints "<n> failed checks"; exit status 1 if any.
//   gather dirs SEED PRIM CHUNK MX MY MZ MODE D POWER RAYDIR FIRSTDIR SECONDDIR USIGN
//                          the 64 directions of chunk CHUNK of primitive PRIM under rng seed SEED, normal (MX, MY, MZ)
//                          (hex floats are read as they are), one "x y z" line of hex floats each: what
//                          vr_debug_gather_samples must return bit for bit.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>

#include "vr_gather.hpp"

using namespace vr;

static int failed = 0;
static long checks = 0;
#define CHECK(cond, ...)                                                                                               \
  do {                                                                                                                 \
    ++checks;                                                                                                          \
    if (!(cond)) {                                                                                                     \
      ++failed;                                                                                                        \
      std::printf("FAILED %s:%d %s | ", __FILE__, __LINE__, #cond);                                                    \
      std::printf(__VA_ARGS__);                                                                                        \
      std::printf("\n");                                                                                               \
    }                                                                                                                  \
  } while (0)

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

static void weight_table() {
  const float NaN = std::numeric_limits<float>::quiet_NaN();
  for (int D = 2; D <= 3; ++D) {
    // n == 1: exactly g = 1, whatever c
    const float g1 = gather_g(1.f, D);
    CHECK(same_bits(g1, 1.f), "g_%d(1) = %a", D, g1);
    for (float c : {1.f, 0.5f, 1e-3f, 1e-30f})
      CHECK(same_bits(gather_weight(GATHER_END_MISS, GATHER_NORMAL, g1, 1.f, c, 0.3f, false, 0.f), 1.f), "D %d c %g", D, c);
    // n = 8
    const float g8 = gather_g(8.f, D);
    const double ref8 = D == 3 ? 4.5 : 2. / (std::sqrt(3.14159265358979323846) * std::tgamma(4.5) / std::tgamma(5.));
    CHECK(std::fabs(g8 - ref8) <= 1e-6 * ref8, "g_%d(8) = %.9g, %.9g", D, g8, ref8);
    for (float c : {1.f, 0.9f, 0.5f, 0.01f}) {
      const float w = gather_weight(GATHER_END_MISS, GATHER_NORMAL, g8, 8.f, c, 0.3f, false, 0.f);
      const double ref = ref8 * std::pow((double)c, 7.);
      CHECK(std::fabs(w - ref) <= 2e-6 * ref, "D %d c %g: %.9g, %.9g", D, c, w, ref);
      CHECK(w <= g8, "the weight is bounded by g");
    }
    for (uint32_t mode : {GATHER_NORMAL, GATHER_SOURCE}) {
      const float n = 8.f, g = gather_g(n, D);
      for (bool em : {false, true}) {
        // c <= 0: nothing, whatever the outcome
        for (float c : {0.f, -0.f, -0.5f, NaN})
          CHECK(gather_weight(GATHER_END_MISS, mode, g, n, c, 0.7f, em, 0.25f) == 0.f, "mode %u c %g", mode, c);
        for (int end : {GATHER_END_IGNORED, GATHER_END_WALL, GATHER_END_BACK})
          for (float c : {0.8f, -0.8f})
            CHECK(gather_weight(end, mode, g, n, c, 0.7f, em, 0.25f) == 0.f, "mode %u end %d c %g", mode, end, c);
        // a front-side hit passes the emission through, with a table only (SOURCE is refused a table by the entry points;
        // the rule itself does not look at the mode)
        for (float c : {0.8f, -0.8f}) {
          const float w = gather_weight(GATHER_END_FRONT, mode, g, n, c, 0.7f, em, 0.25f);
          CHECK(same_bits(w, em ? 0.25f : 0.f), "mode %u front em %d c %g: %g", mode, (int)em, c, w);
        }
      }
    }
    // SOURCE reaching the source: max(0, m . w) / c
    const float g = gather_g(8.f, D);
    CHECK(same_bits(gather_weight(GATHER_END_MISS, GATHER_SOURCE, g, 8.f, 0.8f, 0.6f, false, 0.f), 0.6f / 0.8f), "m.w / c");
    CHECK(gather_weight(GATHER_END_MISS, GATHER_SOURCE, g, 8.f, 0.8f, 0.f, false, 0.f) == 0.f, "m.w = 0");
    CHECK(gather_weight(GATHER_END_MISS, GATHER_SOURCE, g, 8.f, 0.8f, -0.6f, false, 0.f) == 0.f, "m.w < 0");
    CHECK(same_bits(gather_weight(GATHER_END_MISS, GATHER_SOURCE, g, 8.f, 1.f, 1.f, false, 0.f), 1.f), "facing the source");
  }
  CHECK(same_bits(gather_g(3.f, 3), 2.f), "g_3(3)");
  CHECK(std::fabs(gather_g(2.f, 2) - 4. / 3.14159265358979323846) < 1e-7, "g_2(2) = 4 / pi: %.9g", gather_g(2.f, 2));
}

static void quantisation() {
  const int64_t one = (int64_t)1 << GATHER_FRAC_BITS;
  const float M = gather_wmax(4096);
  CHECK(same_bits(M, 1024.f) && same_bits(gather_wmax(1), 4194304.f) && same_bits(gather_wmax(64), 65536.f) &&
            same_bits(gather_wmax(65), 32768.f) && same_bits(gather_wmax(0xFFFFFFFFu), std::ldexp(1.f, -10)),
        "wmax = 2^22 / samples rounded up to a power of two");
  CHECK(gather_q(1.f, M) == one, "q(1)");
  CHECK(gather_q(0.25f, M) == one / 4, "q(1/4)");
  CHECK(gather_q(0.f, M) == 0 && gather_q(-1.f, M) == 0 && gather_q(std::numeric_limits<float>::quiet_NaN(), M) == 0, "q of nothing");
  CHECK(gather_q(std::numeric_limits<float>::infinity(), M) == one << 10 && gather_q(3e7f, M) == one << 10, "q clamps at wmax");
  CHECK(gather_q(std::ldexp(1.f, -41), M) == 1 && gather_q(std::ldexp(1.f, -42), M) == 0, "q rounds to nearest");
  for (uint32_t K : {1u, 64u, 65u, 4096u, 1u << 20, 0xFFFFFFFFu}) // K samples of the largest weight fit an int64 with room
    CHECK((double)K * (double)gather_q(std::numeric_limits<float>::infinity(), gather_wmax(K)) <= std::ldexp(1., 62), "K %u", K);
  for (uint32_t K : {1u, 64u, 65u, 4096u}) {
    const float m = gather_wmax(K);
    int64_t s = 0;
    for (uint32_t k = 0; k < K; ++k)
      s += gather_q(1.f, m);
    CHECK(same_bits(gather_result(s, K), 1.f), "K %u ones", K);
    CHECK(same_bits(gather_result(0, K), 0.f), "K %u zeros", K);
    const float w = 0.3f;
    CHECK(same_bits(gather_result((int64_t)K * gather_q(w, m), K), (float)((double)gather_q(w, m) / (double)one)), "K %u x 0.3", K);
    // one sample in K
    CHECK(std::fabs(gather_result(gather_q(1.f, m), K) - 1. / K) <= 1e-7 / K, "K %u, one hit", K);
  }
}

static void power_guard(std::mt19937_64 &eng) {
  std::uniform_real_distribution<float> U(0.f, 1.f);
  for (float e : {0.5f, 1.f, 7.f, 49.f, 1e4f}) {
    for (int k = 0; k < 20000; ++k) {
      const float c = k % 2 ? U(eng) : 1.f - 0.01f * U(eng);
      if (!(c > 0.f))
        continue;
      const float got = gather_pow(c, e);
      const double ref = std::pow((double)c, (double)e);
      CHECK(ref < 1e-37 ? got <= 2e-37f : std::fabs(got - ref) <= 2e-6 * ref, "pow(%a, %g) = %g, %g", c, e, got, ref);
    }
  }
  // the corners the guard is for: no overflow of the exponent arithmetic, a plain 0
  CHECK(gather_pow(1e-30f, 1e6f) == 0.f && gather_pow(0.999999f, 1e9f) == 0.f && gather_pow(0.5f, 1e30f) == 0.f, "underflow");
  CHECK(gather_pow(1e-45f, 0.5f) == 0.f && gather_pow(1.f, 1e9f) == 1.f && gather_pow(1.0000001f, 7.f) == 1.f, "ends");
  CHECK(std::fabs(gather_pow(0.999999f, 1e5f) - std::pow((double)0.999999f, 1e5)) < 1e-5, "a large power that survives");
}

static double len_of(const GVec &v) { return std::sqrt((double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z); }

static void directions(std::mt19937_64 &eng) {
  const int N = 100000;
  const double ulp2 = 2. * std::ldexp(1., -23);
  const GatherFrame frames[] = {{2, 0, 1, 1.f}, {2, 0, 1, -1.f}, {1, 0, 2, 1.f}, {0, 1, 2, -1.f}};
  GVec normals[] = {{0.f, 0.f, 1.f}, {0.f, 0.f, -1.f}, {1.f, 0.f, 0.f}, {0.f, -1.f, 0.f}, {0.3f, -0.5f, 0.8f}, {-0.6f, 0.2f, -0.4f}};
  for (GVec &m : normals)
    gather_normalize(m);
  // NORMAL, D = 3
  for (const GVec &m : normals) {
    double mean = 0., worst = 0.;
    long below = 0;
    for (int k = 0; k < N; ++k) {
      const float r1 = gather_canon(eng()), r2 = gather_canon(eng());
      const GVec w = gather_direction(GATHER_NORMAL, 3, r1, r2, m, 1.f, frames[0]);
      worst = std::fmax(worst, std::fabs(len_of(w) - 1.));
      const float d = gather_dot(m, w);
      below += !(d > 0.f);
      mean += d;
    }
    mean /= N;
    CHECK(worst <= ulp2, "NORMAL 3-D |w| - 1 = %g", worst);
    CHECK(below == 0, "NORMAL 3-D: %ld samples with m . w <= 0", below);
    CHECK(std::fabs(mean - 2. / 3.) <= 5. * std::sqrt(1. / 18.) / std::sqrt((double)N), "NORMAL 3-D mean m . w = %.6f", mean);
  }
  // NORMAL, D = 2: in the plane, about m; mean m . w = pi / 4 (variance 2/3 - pi^2/16 < 1/18)
  for (GVec m : {GVec{0.f, 1.f, 0.f}, GVec{1.f, 0.f, 0.f}, GVec{-0.6f, 0.8f, 0.f}, GVec{0.28f, -0.96f, 0.f}}) {
    double mean = 0., worst = 0.;
    long below = 0, offPlane = 0;
    for (int k = 0; k < N; ++k) {
      const float r1 = gather_canon(eng()), r2 = gather_canon(eng());
      const GVec w = gather_direction(GATHER_NORMAL, 2, r1, r2, m, 1.f, frames[2]);
      worst = std::fmax(worst, std::fabs(len_of(w) - 1.));
      const float d = gather_dot(m, w);
      below += !(d > 0.f);
      offPlane += w.z != 0.f;
      mean += d;
    }
    mean /= N;
    CHECK(worst <= ulp2, "NORMAL 2-D |w| - 1 = %g", worst);
    CHECK(below == 0 && offPlane == 0, "NORMAL 2-D: %ld with m . w <= 0, %ld off the plane", below, offPlane);
    CHECK(std::fabs(mean - 0.78539816339744831) <= 5. * std::sqrt(1. / 18.) / std::sqrt((double)N), "NORMAL 2-D mean m . w = %.6f", mean);
  }
  // SOURCE, D = 3: mean c = (n + 1) / (n + 2), sigma^2 <= 1/4
  for (const GatherFrame &f : frames) {
    for (float n : {2.f, 8.f, 50.f}) {
      double mean = 0., worst = 0.;
      long below = 0;
      for (int k = 0; k < N; ++k) {
        const float r1 = gather_canon(eng()), r2 = gather_canon(eng());
        const GVec w = gather_direction(GATHER_SOURCE, 3, r1, r2, normals[4], n, f);
        worst = std::fmax(worst, std::fabs(len_of(w) - 1.));
        const float c = gather_c(w, f);
        below += !(c >= 0.f);
        mean += c;
      }
      mean /= N;
      CHECK(worst <= ulp2, "SOURCE 3-D n %g |w| - 1 = %g", n, worst);
      CHECK(below == 0, "SOURCE 3-D: %ld samples with c < 0", below);
      CHECK(std::fabs(mean - (n + 1.) / (n + 2.)) <= 5. * 0.5 / std::sqrt((double)N), "SOURCE 3-D n %g mean c = %.6f", n, mean);
    }
  }
  // SOURCE, D = 2 (tracing axis y, plane axes x and z): z dropped, the rest normalised
  for (float n : {2.f, 8.f}) {
    double worst = 0.;
    long bad = 0;
    for (int k = 0; k < N; ++k) {
      const float r1 = gather_canon(eng()), r2 = gather_canon(eng());
      const GVec w = gather_direction(GATHER_SOURCE, 2, r1, r2, normals[4], n, frames[2]);
      if (w.x == 0.f && w.y == 0.f)
        continue; // (cos(theta) = 0 and an azimuth along z: nothing left to normalise; never walked: c = 0)
      worst = std::fmax(worst, std::fabs(len_of(w) - 1.));
      bad += w.z != 0.f || !(gather_c(w, frames[2]) >= 0.f);
    }
    CHECK(worst <= ulp2 && bad == 0, "SOURCE 2-D n %g |w| - 1 = %g, %ld off the plane or below it", n, worst, bad);
  }
  // the triangle centroid from the packed record
  const GVec v0{1.f, 2.f, 3.f}, v1{4.f, 0.f, 3.5f}, v2{-2.f, 5.f, 1.f};
  const GVec c = gather_tri_centroid(v0, GVec{v0.x - v1.x, v0.y - v1.y, v0.z - v1.z}, GVec{v2.x - v0.x, v2.y - v0.y, v2.z - v0.z});
  CHECK(same_bits(c.x, 1.f) && std::fabs(c.y - 7.f / 3.f) < 1e-6f && same_bits(c.z, 2.5f), "centroid %g %g %g", c.x, c.y, c.z);
}

static int print_dirs(char **v) {
  const uint32_t seed = (uint32_t)std::strtoul(v[0], nullptr, 0), prim = (uint32_t)std::strtoul(v[1], nullptr, 0),
                 chunk = (uint32_t)std::strtoul(v[2], nullptr, 0);
  const GVec m{std::strtof(v[3], nullptr), std::strtof(v[4], nullptr), std::strtof(v[5], nullptr)};
  const uint32_t mode = (uint32_t)std::strtoul(v[6], nullptr, 0);
  const int D = std::atoi(v[7]);
  const float n = std::strtof(v[8], nullptr);
  const GatherFrame f{std::atoi(v[9]), std::atoi(v[10]), std::atoi(v[11]), std::strtof(v[12], nullptr)};
  std::mt19937_64 eng(gather_chunk_seed(prim, seed, chunk));
  for (uint32_t j = 0; j < GATHER_CHUNK; ++j) {
    const float r1 = gather_canon(eng()), r2 = gather_canon(eng());
    const GVec w = gather_direction(mode, D, r1, r2, m, n, f);
    std::printf("%a %a %a\n", w.x, w.y, w.z);
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 15 && std::strcmp(argv[1], "dirs") == 0)
    return print_dirs(argv + 2);
  if (argc != 1) {
    std::fprintf(stderr, "usage: gather | gather dirs SEED PRIM CHUNK MX MY MZ MODE D POWER RAYDIR FIRSTDIR SECONDDIR USIGN\n");
    return 2;
  }
  std::mt19937_64 eng(20240607u);
  weight_table();
  quantisation();
  power_guard(eng);
  directions(eng);
  std::printf("%ld checks\n%d failed checks\n", checks, failed);
  return failed ? 1 : 0;
}
