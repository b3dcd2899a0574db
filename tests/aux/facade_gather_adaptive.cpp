// Trace::gatherFluxAdaptive / gatherPathsAdaptive / gatherAdaptiveDevice / gatherSums: the gather to a target error through
// the façade, on the folded sheet of facade_gather_paths.cpp.  Checks: a huge target is gatherFlux(minSamples) word for word
// with every primitive at minSamples, target 0 is gatherFlux(maxSamples) with every primitive at maxSamples, totalSamples is
// the sum of samplesUsed, the sums over chunks [0, K / 64) divide to gatherFlux(K), the device form over two ranges is the
// host form, refusals come back empty, an adaptive gather leaves the flux of the apply as it was.
// Prints "facade gather adaptive ok" when everything holds.
#include <hip/hip_runtime_api.h>

#include <rayBoundary.hpp>
#include <rayParticle.hpp>
#include <rayTraceDisk.hpp>

#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

using namespace viennaray;

static int fail(const char *what) {
  std::printf("FAILED: %s\n", what);
  return 1;
}

int main() {
  constexpr int N = 16;
  std::vector<std::array<float, 3>> points, normals;
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) {
      const int k = i % 8;
      const double s = k < 4 ? -1. : 1.;
      points.push_back({(float)i, (float)j, 1.5f * (float)std::abs(k - 4)});
      normals.push_back({(float)(-s * 1.5 / std::sqrt(3.25)), 0.f, (float)(1. / std::sqrt(3.25))});
    }

  TraceDisk<float, 3> tracer;
  tracer.setGeometry(points, normals, 1.f);
  BoundaryCondition bcs[3] = {BoundaryCondition::PERIODIC_BOUNDARY, BoundaryCondition::PERIODIC_BOUNDARY,
                              BoundaryCondition::PERIODIC_BOUNDARY};
  tracer.setBoundaryConditions(bcs);
  tracer.setNumberOfRaysFixed(20000);
  tracer.setUseRandomSeeds(false);
  tracer.setRngSeed(7);
  auto particle = std::make_unique<DiffuseParticle<float, 3>>(0.3f, "flux");
  tracer.setParticleType(particle);

  if (!tracer.gatherFluxAdaptive(0.05f).flux.empty())
    return fail("an adaptive gather before any apply must be refused");
  tracer.apply();
  if (tracer.getRayTraceInfo().error)
    return fail("apply");
  const std::vector<float> flux = tracer.getLocalData().getVectorData(0);
  const size_t n = points.size();

  const auto coarse = tracer.gatherFluxAdaptive(std::numeric_limits<float>::infinity(), 64, 256);
  if (coarse.flux != tracer.gatherFlux(64) || coarse.samplesUsed != std::vector<unsigned>(n, 64u) || coarse.info.rounds != 1u)
    return fail("a huge target is gatherFlux(minSamples)");
  const auto fine = tracer.gatherFluxAdaptive(0.f, 64, 256);
  if (fine.flux != tracer.gatherFlux(256) || fine.samplesUsed != std::vector<unsigned>(n, 256u) || fine.info.rounds != 3u ||
      fine.info.unconverged != n)
    return fail("target 0 is gatherFlux(maxSamples)");
  const auto paths = tracer.gatherPathsAdaptive(0.05f, 0.3f, GatherReflection::SPECULAR, 8, 64, 1024);
  if (paths.flux.size() != n || paths.stdErr.size() != n)
    return fail("gatherPathsAdaptive");
  unsigned long long total = 0;
  for (unsigned k : paths.samplesUsed) {
    if (k < 64u || k > 1024u || (k & (k - 1u)))
      return fail("samplesUsed is minSamples times a power of two up to maxSamples");
    total += k;
  }
  if (total != paths.info.totalSamples)
    return fail("totalSamples is the sum of samplesUsed");

  std::vector<int64_t> s1, s2;
  vr_gather_spec spec{};
  spec.cosinePower = 1.f;
  if (!tracer.gatherSums(spec, 0, 4, 256, s1, s2) || s1.size() != n)
    return fail("gatherSums");
  for (size_t i = 0; i < n; ++i)
    if ((float)((double)s1[i] / 1099511627776.0 / 256.) != fine.flux[i] || s2[i] != (s1[i] >> 12))
      return fail("the sums divide to gatherFlux(K); unit weights square to sum >> 12");

  if (!tracer.gatherFluxAdaptive(0.05f, 96, 192).flux.empty() || !tracer.gatherFluxAdaptive(0.05f, 64, 192).flux.empty() ||
      !tracer.gatherFluxAdaptive(std::nanf(""), 64, 256).flux.empty() || !tracer.gatherFluxAdaptive(-1.f, 64, 256).flux.empty() ||
      tracer.gatherSums(spec, 3, 2, 256, s1, s2))
    return fail("minSamples 96, maxSamples 3 x min, a NaN or negative target, chunks beyond the budget must be refused");
  if (tracer.getLocalData().getVectorData(0) != flux)
    return fail("the flux after an adaptive gather");

  float *dFlux = nullptr, *dErr = nullptr;
  uint32_t *dUsed = nullptr;
  if (hipMalloc((void **)&dFlux, n * 4) != hipSuccess || hipMalloc((void **)&dErr, n * 4) != hipSuccess ||
      hipMalloc((void **)&dUsed, n * 4) != hipSuccess)
    return fail("hipMalloc");
  const unsigned third = (unsigned)n / 3;
  const vr_gather_spec pspec = tracer.pathsSpec(nullptr, 1.f - 0.3f, GatherReflection::SPECULAR, 8);
  vr_gather_adaptive_info ia{}, ib{};
  std::vector<float> gotFlux(n), gotErr(n);
  std::vector<unsigned> gotUsed(n);
  if (!tracer.gatherAdaptiveDevice(pspec, 0, third, 64, 1024, 0.05f, 0.f, dFlux, dErr, dUsed, ia) ||
      !tracer.gatherAdaptiveDevice(pspec, third, (unsigned)n - third, 64, 1024, 0.05f, 0.f, dFlux + third, dErr + third, dUsed + third,
                                   ib) ||
      hipDeviceSynchronize() != hipSuccess || hipMemcpy(gotFlux.data(), dFlux, n * 4, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(gotErr.data(), dErr, n * 4, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(gotUsed.data(), dUsed, n * 4, hipMemcpyDeviceToHost) != hipSuccess)
    return fail("gatherAdaptiveDevice");
  if (std::memcmp(gotFlux.data(), paths.flux.data(), n * 4) || std::memcmp(gotErr.data(), paths.stdErr.data(), n * 4) ||
      gotUsed != paths.samplesUsed || ia.totalSamples + ib.totalSamples != paths.info.totalSamples ||
      ia.unconverged + ib.unconverged != paths.info.unconverged)
    return fail("the device form over two ranges differs from the host form");
  if (tracer.gatherAdaptiveDevice(pspec, 0, (unsigned)n, 64, 1024, 0.05f, 0.f, gotFlux.data(), nullptr, nullptr, ia))
    return fail("a host pointer must be refused");
  (void)hipFree(dFlux);
  (void)hipFree(dErr);
  (void)hipFree(dUsed);
  std::printf("facade gather adaptive ok\n");
  return 0;
}
