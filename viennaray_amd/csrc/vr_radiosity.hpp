// vr_radiosity.hpp — the arithmetic of solveRadiosity (vr_radiosity.hip: the iteration over a recorded link table) in
// plain C++, in the manner of vr_gather.hpp: the host compiler takes this file and vr_gather.hpp alone
// (tests/aux/radiosity.cpp), the kernels include it.  What the link table's index is, what a row of one iteration
// computes, the reflectivity multiply and the residual live here, so that the host program and the device compute the
// same bits from the same text.  include/viennaray_amd.h has the definition this implements.
#pragma once
#include <cstdint>

#include "vr_gather.hpp"

namespace vr {

constexpr int32_t RADIOSITY_NO_LINK = -1; // the sample brings nothing back from the surface (it may have reached the source)

// The link table: sample-major over the scene's leaf (packed, Morton) slots, a row of `slots` int32 per sample.
// slots: the primitive count rounded up to whole waves, so that every wave's store of one sample is one aligned
// 256-byte line and every row starts on one.  64-bit throughout: 10^6 primitives x 4096 samples is 4 x 10^9 entries
VR_GATHER_FN uint64_t radiosity_slots(uint32_t numPrims) { return (((uint64_t)numPrims + 63u) / 64u) * 64u; }
VR_GATHER_FN uint64_t radiosity_link_count(uint32_t numPrims, uint32_t samples) {
  return radiosity_slots(numPrims) * (uint64_t)samples;
}
// the entry of sample `sample` (< samples) of the primitive at leaf position `slot` (< slots)
VR_GATHER_FN uint64_t radiosity_link_index(uint64_t slots, uint32_t slot, uint32_t sample) {
  return (uint64_t)sample * slots + (uint64_t)slot;
}

// what one link adds to a row's int64 sum: q(e[link]) for a front-side hit, nothing otherwise.  e is indexed by whatever
// the links hold (the device: leaf positions, with e in leaf order)
VR_GATHER_FN int64_t radiosity_link_q(int32_t link, const float *e, float wmax) {
  return link >= 0 ? gather_q(e[link], wmax) : 0;
}
// F of a row from its direct sum and the sum over its links
VR_GATHER_FN float radiosity_row_result(int64_t direct, int64_t linkSum, uint32_t samples) {
  return gather_result(direct + linkSum, samples);
}
// e_{t+1}[j] = rho[j] F_t[j]: one float32 multiply
VR_GATHER_FN float radiosity_emission(float rho, float F) { return rho * F; }
// |F_t - F_{t-1}| as the word the maximum is taken over: one float32 subtraction, the sign bit cleared.  For
// non-negative floats (NaN cannot occur: F is finite) the order of the words is the order of the values, so an integer
// maximum in any order gives the float maximum
VR_GATHER_FN uint32_t radiosity_residual_bits(float now, float before) {
  const float d = now - before;
  return vr_asuint(d) & 0x7fffffffu;
}
VR_GATHER_FN float radiosity_residual_value(uint32_t bits) { return vr_asfloat(bits); }
// the reflectivity a solve accepts: 0 <= rho <= 1 (NaN fails both comparisons)
VR_GATHER_FN bool radiosity_rho_ok(float rho) { return rho >= 0.f && rho <= 1.f; }
// the stopping rule: after iteration t >= 1 with residual r
VR_GATHER_FN bool radiosity_stops(uint32_t residualBits, float tolerance) {
  return radiosity_residual_value(residualBits) <= tolerance;
}

// The whole solve over one table on the host — the reference the device is held to, and what tests/aux/radiosity.cpp
// runs: links[radiosity_link_index(slots, i, k)] index e directly.  F, e0, e1: n floats each.  Returns t; *residual: r_t
// (0 for t == 0)
inline uint32_t radiosity_solve_host(const int32_t *links, const int64_t *direct, uint32_t n, uint32_t samples, const float *rho,
                                     float tolerance, uint32_t maxIterations, float *F, float *e0, float *e1, float *residual) {
  const uint64_t slots = radiosity_slots(n);
  const float wmax = gather_wmax(samples);
  for (uint32_t i = 0; i < n; ++i) {
    F[i] = radiosity_row_result(direct[i], 0, samples);
    e0[i] = radiosity_emission(rho[i], F[i]);
  }
  *residual = 0.f;
  uint32_t t = 0;
  while (t < maxIterations) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < n; ++i) {
      int64_t sum = 0;
      for (uint32_t k = 0; k < samples; ++k)
        sum += radiosity_link_q(links[radiosity_link_index(slots, i, k)], e0, wmax);
      const float f = radiosity_row_result(direct[i], sum, samples);
      const uint32_t b = radiosity_residual_bits(f, F[i]);
      r = b > r ? b : r;
      F[i] = f;
      e1[i] = radiosity_emission(rho[i], f);
    }
    ++t;
    *residual = radiosity_residual_value(r);
    float *const s = e0;
    e0 = e1;
    e1 = s;
    if (radiosity_stops(r, tolerance))
      break;
  }
  return t;
}

} // namespace vr
