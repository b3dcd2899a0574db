// uniform_disk_threshold (viennaray_amd/csrc/vr_uniform_disks.hpp) on the host: for every radius of the table and every
// input x below, (radius > sqrtf(x)) == (x < T) — the comparison the uniform-disk neighbour test makes in place of the
// square root.  Inputs per radius: every float within 65 536 ulps of radius^2 on either side, 10^7 random positive floats
// (random bit patterns: every binade alike), and +0, +infinity, a NaN.  T itself must be the SMALLEST float whose square
// root reaches the radius.  Prints one line per radius and "N failed checks"; exit status 1 if N > 0.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>

#include "../../viennaray_amd/csrc/vr_uniform_disks.hpp"

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

int main() {
  const float root34 = 0.8660254f; // the disk radius of a level-set cloud in units of gridDelta
  const float radii[] = {root34 * 1.f, root34 * 0.5f, root34 * 0.01f, root34 * 37.3f, 1.0f, std::ldexp(1.f, -20), 3e18f};
  unsigned long long failed = 0, checked = 0;
  std::mt19937 rng(20240229u);
  for (const float radius : radii) {
    const float T = vr::uniform_disk_threshold(radius);
    unsigned long long bad = 0, n = 0;
    auto check = [&](float x) {
      ++n;
      if ((radius > std::sqrt(x)) != (x < T)) {
        if (bad < 5)
          std::printf("  radius %.9g (T %.9g): x %.9g (bits %08x) sqrt %.9g\n", radius, T, x, to_bits(x), std::sqrt(x));
        ++bad;
      }
    };
    // T is the smallest float whose square root reaches the radius
    if (!(std::sqrt(T) >= radius) || !(T > 0.f) || std::sqrt(std::nextafter(T, 0.f)) >= radius) {
      std::printf("  radius %.9g: T %.9g is not the smallest float with sqrtf(T) >= radius\n", radius, T);
      ++bad;
    }
    const uint32_t mid = to_bits(radius * radius); // (positive floats: consecutive bit patterns are consecutive floats)
    for (int64_t k = -65536; k <= 65536; ++k) {
      const int64_t b = (int64_t)mid + k;
      if (b >= 0 && b <= 0x7F800000ll)
        check(from_bits((uint32_t)b));
    }
    for (int k = 0; k < 10000000; ++k) {
      uint32_t b = rng() & 0x7FFFFFFFu;
      if (b > 0x7F800000u)
        b &= 0x7F7FFFFFu; // (a NaN pattern: make it finite; NaN has its own check below)
      if (b == 0u)
        b = 1u;
      check(from_bits(b));
    }
    check(0.f);
    check(std::numeric_limits<float>::infinity());
    check(std::numeric_limits<float>::quiet_NaN());
    std::printf("radius %.9g  T %.9g (radius^2 %+d ulps)  %llu inputs  %llu mismatches\n", radius, T,
                (int)((int64_t)to_bits(T) - (int64_t)mid), n, bad);
    failed += bad;
    checked += n;
  }
  // radii that are no disk's: nothing is below them, or every finite x is
  if (vr::uniform_disk_threshold(0.f) != 0.f || vr::uniform_disk_threshold(-1.f) != 0.f ||
      vr::uniform_disk_threshold(std::numeric_limits<float>::quiet_NaN()) != 0.f ||
      vr::uniform_disk_threshold(std::numeric_limits<float>::infinity()) != std::numeric_limits<float>::infinity() ||
      vr::uniform_disk_threshold(3e19f) != std::numeric_limits<float>::infinity()) {
    std::printf("  a degenerate radius has the wrong threshold\n");
    ++failed;
  }
  std::printf("%llu inputs\n%llu failed checks\n", checked, failed);
  return failed ? 1 : 0;
}
