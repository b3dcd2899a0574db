// The arithmetic of gatherPaths (viennaray_amd/csrc/vr_gather.hpp: the counter draw, the throughput update, the end -> weight
// rule; viennaray_amd/csrc/vr_math.hpp: reflect_specular) on the host: the headers the kernel includes, taken by the host
// compiler alone.
//   gather_paths                  the checks.  Prints "<n> checks" and "<n> failed checks"; exit status 1 if any failed.
//   gather_paths stats SEED       over 2^16 draws (256 primitives x 64 samples x 4 bounces): "<mean r> <mean r1 r2> <min> <max>"
//   gather_paths draws SEED PRIM SAMPLE COUNT
//                                 "r1 r2" (hex floats) of bounces 0 .. COUNT - 1 of that path
//   gather_paths dirs SEED D      reads lines "PRIM SAMPLE BOUNCE NX NY NZ" (hex floats are read as they are) and prints the
//                                 direction a DIFFUSE vertex leaves along, "x y z" in hex floats: what
//                                 vr_debug_gather_path must return bit for bit
//   gather_paths weights D POWER  reads lines "END C T" (the end code, c_end and T as hex floats) and prints the weight
//   gather_paths reflect          reads lines "DX DY DZ NX NY NZ" and prints reflect_specular(d, n) in hex floats
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "vr_gather.hpp"

#include "vr_math.hpp"

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

static void draws() {
  // a pure function of its four inputs, in [0, 1), different between neighbouring samples and bounces
  for (uint32_t seed : {0u, 7u, 0xFFFFFFFFu})
    for (uint32_t prim : {0u, 1u, 639u, 1000000u, 0xFFFFFFFEu})
      for (uint32_t sample = 0; sample < 130; ++sample)
        for (uint32_t bounce = 0; bounce < 20; ++bounce) {
          float a1, a2, b1, b2;
          gather_path_draw(seed, prim, sample, bounce, a1, a2);
          gather_path_draw(seed, prim, sample, bounce, b1, b2);
          CHECK(same_bits(a1, b1) && same_bits(a2, b2), "not pure");
          CHECK(a1 >= 0.f && a1 < 1.f && a2 >= 0.f && a2 < 1.f, "r1 %a r2 %a", a1, a2);
          CHECK(!same_bits(a1, a2), "r1 == r2 at %u %u %u %u", seed, prim, sample, bounce);
          gather_path_draw(seed, prim, sample + 1u, bounce, b1, b2);
          CHECK(!same_bits(a1, b1) || !same_bits(a2, b2), "the next sample draws the same");
          gather_path_draw(seed, prim, sample, bounce + 1u, b1, b2);
          CHECK(!same_bits(a1, b1) || !same_bits(a2, b2), "the next bounce draws the same");
          gather_path_draw(seed, prim + 1u, sample, bounce, b1, b2);
          CHECK(!same_bits(a1, b1) || !same_bits(a2, b2), "the next primitive draws the same");
          gather_path_draw(seed + 1u, prim, sample, bounce, b1, b2);
          CHECK(!same_bits(a1, b1) || !same_bits(a2, b2), "the next seed draws the same");
        }
  // the largest hash gives the largest float below 1
  CHECK(same_bits((float)(0xFFFFFFFFu >> 8) * 5.9604644775390625e-08f, 0.99999994f), "2^-24 (2^24 - 1)");
  // the diffuse direction: unit length, in the hemisphere of the normal
  const GVec normals[] = {{0.f, 0.f, 1.f}, {1.f, 0.f, 0.f}, {-1.f, 0.f, 0.f}, {0.6f, 0.f, 0.8f}, {0.f, -1.f, 0.f}};
  for (int D = 2; D <= 3; ++D)
    for (const GVec &n : normals) {
      if (D == 2 && n.z != 0.f)
        continue;
      for (uint32_t sample = 0; sample < 500; ++sample) {
        const GVec d = gather_path_diffuse(D, 7u, 11u, sample, sample % 5u, n);
        CHECK(std::fabs(std::sqrt((double)d.x * d.x + (double)d.y * d.y + (double)d.z * d.z) - 1.) < 3e-7, "length");
        CHECK(gather_dot(d, n) >= 0.f, "hemisphere");
      }
    }
}

static void throughput_and_ends() {
  const float NaN = std::numeric_limits<float>::quiet_NaN();
  CHECK(same_bits(gather_path_throughput(1.f, 0.7f), 0.7f), "T = 1");
  CHECK(same_bits(gather_path_throughput(0.7f, 0.7f), 0.7f * 0.7f), "one multiply");
  CHECK(gather_path_throughput(0.3f, 0.f) == 0.f, "rho 0");
  CHECK(gather_path_rho_ok(0.f) && gather_path_rho_ok(1.f) && gather_path_rho_ok(0.5f), "accepted");
  CHECK(!gather_path_rho_ok(NaN) && !gather_path_rho_ok(-1e-9f) && !gather_path_rho_ok(1.0000001f), "refused");
  for (int D = 2; D <= 3; ++D)
    for (float n : {1.f, 8.f, 50.f}) {
      const float g = gather_g(n, D);
      for (float c : {1.f, 0.9f, 0.3f, 1e-3f, 0.f, -0.4f, NaN}) {
        // T = 1 leaves the gather's weight bit for bit
        const float w = gather_weight(GATHER_END_MISS, GATHER_NORMAL, g, n, c, 0.f, false, 0.f);
        CHECK(same_bits(gather_path_weight(GATHER_END_MISS, g, n, c, 1.f), w), "T = 1, n %g c %g", n, c);
        CHECK(same_bits(gather_path_weight(GATHER_END_MISS, g, n, c, 0.49f), w * 0.49f), "one multiply by T");
        CHECK(gather_path_weight(GATHER_END_MISS, g, n, c, 0.f) == 0.f || !(c > 0.f), "T = 0");
        CHECK(gather_q(gather_path_weight(GATHER_END_MISS, g, n, c, 0.f), 1024.f) == 0, "T = 0 counts nothing");
        for (int end : {(int)GATHER_END_IGNORED, (int)GATHER_END_WALL, (int)GATHER_END_FRONT, (int)GATHER_END_BACK, GATHER_END_BOUNCES,
                        GATHER_END_ABSORBED})
          for (float T : {1.f, 0.5f, 0.f})
            CHECK(same_bits(gather_path_weight(end, g, n, c, T), 0.f), "end %d", end);
      }
    }
}

// numpy float32, one operation at a time, in the header's order
static void reflect_checks() {
  const float d[][3] = {{0.3f, 0.2f, -0.9f}, {-0.70710678f, 0.f, -0.70710678f}, {0.1f, -0.995f, 0.f}, {0.f, 0.f, -1.f}};
  const float n[][3] = {{0.f, 0.f, 1.f}, {1.f, 0.f, 0.f}, {0.6f, 0.f, 0.8f}, {-0.26726124f, 0.53452248f, 0.80178373f}};
  for (auto &dv : d)
    for (auto &nv : n) {
      const V3 r = reflect_specular(V3{dv[0], dv[1], dv[2]}, V3{nv[0], nv[1], nv[2]});
      volatile float ix = -dv[0], iy = -dv[1], iz = -dv[2];
      volatile float a = nv[0] * ix, b = nv[1] * iy, s = a + b, e = nv[2] * iz, dot = s + e, f = 2.f * dot;
      volatile float px = f * nv[0], py = f * nv[1], pz = f * nv[2];
      volatile float rx = px - ix, ry = py - iy, rz = pz - iz;
      CHECK(same_bits(r.x, rx) && same_bits(r.y, ry) && same_bits(r.z, rz), "reflect_specular");
      const double len = std::sqrt((double)r.x * r.x + (double)r.y * r.y + (double)r.z * r.z);
      const double len0 = std::sqrt((double)dv[0] * dv[0] + (double)dv[1] * dv[1] + (double)dv[2] * dv[2]);
      CHECK(std::fabs(len - len0) < 1e-6, "a mirror keeps the length: %g %g", len, len0);
    }
}

static float hexf(const char *s) { return std::strtof(s, nullptr); }

int main(int argc, char **argv) {
  if (argc >= 3 && !std::strcmp(argv[1], "stats")) {
    const uint32_t seed = (uint32_t)std::strtoul(argv[2], nullptr, 10);
    double s1 = 0., s12 = 0.;
    float lo = 2.f, hi = -1.f;
    long cnt = 0;
    for (uint32_t prim = 0; prim < 256; ++prim)
      for (uint32_t sample = 0; sample < 64; ++sample)
        for (uint32_t bounce = 0; bounce < 4; ++bounce, ++cnt) {
          float r1, r2;
          gather_path_draw(seed, prim, sample, bounce, r1, r2);
          s1 += r1, s12 += (double)r1 * r2;
          lo = std::fmin(lo, std::fmin(r1, r2)), hi = std::fmax(hi, std::fmax(r1, r2));
        }
    std::printf("%.17g %.17g %.9g %.9g %ld\n", s1 / cnt, s12 / cnt, lo, hi, cnt);
    return 0;
  }
  if (argc >= 6 && !std::strcmp(argv[1], "draws")) {
    const uint32_t seed = (uint32_t)std::strtoul(argv[2], nullptr, 10), prim = (uint32_t)std::strtoul(argv[3], nullptr, 10),
                   sample = (uint32_t)std::strtoul(argv[4], nullptr, 10), count = (uint32_t)std::strtoul(argv[5], nullptr, 10);
    for (uint32_t b = 0; b < count; ++b) {
      float r1, r2;
      gather_path_draw(seed, prim, sample, b, r1, r2);
      std::printf("%a %a\n", r1, r2);
    }
    return 0;
  }
  if (argc >= 4 && !std::strcmp(argv[1], "dirs")) {
    const uint32_t seed = (uint32_t)std::strtoul(argv[2], nullptr, 10);
    const int D = std::atoi(argv[3]);
    unsigned prim, sample, bounce;
    char x[64], y[64], z[64];
    while (std::scanf("%u %u %u %63s %63s %63s", &prim, &sample, &bounce, x, y, z) == 6) {
      const GVec d = gather_path_diffuse(D, seed, prim, sample, bounce, GVec{hexf(x), hexf(y), hexf(z)});
      std::printf("%a %a %a\n", d.x, d.y, d.z);
    }
    return 0;
  }
  if (argc >= 4 && !std::strcmp(argv[1], "weights")) { // gather_paths weights D POWER: lines "END C T" -> the weight
    const int D = std::atoi(argv[2]);
    const float n = hexf(argv[3]), g = gather_g(n, D);
    int end;
    char c[64], T[64];
    while (std::scanf("%d %63s %63s", &end, c, T) == 3)
      std::printf("%a\n", gather_path_weight(end, g, n, hexf(c), hexf(T)));
    return 0;
  }
  if (argc >= 2 && !std::strcmp(argv[1], "reflect")) {
    char t[6][64];
    while (std::scanf("%63s %63s %63s %63s %63s %63s", t[0], t[1], t[2], t[3], t[4], t[5]) == 6) {
      const V3 r = reflect_specular(V3{hexf(t[0]), hexf(t[1]), hexf(t[2])}, V3{hexf(t[3]), hexf(t[4]), hexf(t[5])});
      std::printf("%a %a %a\n", r.x, r.y, r.z);
    }
    return 0;
  }
  draws();
  throughput_and_ends();
  reflect_checks();
  std::printf("%ld checks\n%d failed checks\n", checks, failed);
  return failed ? 1 : 0;
}
