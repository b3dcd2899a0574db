// vr_uniform_disks.hpp — the host side of the uniform-disk candidate tests (pq_hit_packet UNIFORM, vr_packet_query.hpp): the
// threshold that replaces the neighbour test's square root.  Host code only (vr_prepare.cpp; tests/aux/uniform_threshold.cpp).
#pragma once
#include <cmath>
#include <limits>

namespace vr {

// The smallest float T with sqrtf(T) >= radius, so that for EVERY float x >= +0, an infinity and a NaN included,
//   radius > sqrtf(x)  <=>  x < T.
// Why: a correctly rounded square root is monotone (x <= y gives sqrtf(x) <= sqrtf(y)).  For x < T, sqrtf(x) < radius by
// the choice of T; for x >= T, sqrtf(x) >= sqrtf(T) >= radius; a NaN fails both comparisons.  The host's sqrtf (IEEE 754,
// correctly rounded) and the device's (the kernels are compiled without fast math: correctly rounded too) agree on every
// input, so the T found here is the device's.  radius * radius is within a few ulps of T: the search steps by ulps.
// A radius that is not positive (or a NaN) is greater than no square root: T = 0, below which no x >= +0 lies.
inline float uniform_disk_threshold(float radius) {
  if (!(radius > 0.f))
    return 0.f;
  const float inf = std::numeric_limits<float>::infinity();
  if (radius == inf)
    return inf; // (every finite x passes, an infinite one does not)
  float x = radius * radius; // (the Makefile's -ffp-contract=off -fno-fast-math: one rounded multiplication)
  if (x == inf)
    x = std::numeric_limits<float>::max();
  while (x > 0.f && std::sqrt(std::nextafter(x, 0.f)) >= radius) // down while the float below still reaches the radius
    x = std::nextafter(x, 0.f);
  while (std::sqrt(x) < radius) // up to the first float that reaches it
    x = std::nextafter(x, inf);
  return x;
}

} // namespace vr
