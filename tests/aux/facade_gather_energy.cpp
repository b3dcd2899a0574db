// Trace::gatherEnergy / gatherEnergyDevice / gatherEnergySums / gatherEnergyAdaptive: the energy gather through the façade,
// on the folded sheet of facade_gather_angular.cpp.  Checks: an all-ones yield is gatherAngular word for word, a constant
// yield of 2 doubles the int64 sums, retention R under yield {0, 1} at sticking 0 is gatherAngular with reflectivity law R,
// the cut changes no sum, the device form over two ranges is the host form, the adaptive call at target 0 is the fixed-K call
// at maxSamples, refusals come back empty, a gather leaves the flux of the apply as it was.
// Prints "facade gather energy ok" when everything holds.
#include <hip/hip_runtime_api.h>

#include <rayBoundary.hpp>
#include <rayParticle.hpp>
#include <rayTraceDisk.hpp>

#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
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

  using Tracer = TraceDisk<float, 3>;
  Tracer tracer;
  tracer.setGeometry(points, normals, 1.f);
  BoundaryCondition bcs[3] = {BoundaryCondition::PERIODIC_BOUNDARY, BoundaryCondition::PERIODIC_BOUNDARY,
                              BoundaryCondition::PERIODIC_BOUNDARY};
  tracer.setBoundaryConditions(bcs);
  tracer.setNumberOfRaysFixed(20000);
  tracer.setUseRandomSeeds(false);
  tracer.setRngSeed(7);
  auto particle = std::make_unique<DiffuseParticle<float, 3>>(0.3f, "flux");
  tracer.setParticleType(particle);

  Tracer::GatherLaws none, mixed, lawR;
  mixed.reflectivity = {1.f, 0.8f, 0.6f, 0.4f, 0.2f};
  mixed.yield = {0.5f, 3.f};
  lawR.reflectivity = {0.3f, 0.5f, 0.9f, 1.f};
  Tracer::GatherEnergy ones, twice, ident, ion, ionNoCut, bad;
  ones.yield.assign(9, 1.f);
  ones.energyMax = 100.f;
  ones.sourceQuantiles = {20.f, 90.f};
  ones.retention = {0.2f, 0.9f};
  twice.yield.assign(2, 2.f);
  ident.yield = {0.f, 1.f};
  ident.energyMax = ident.sourceEnergy = 1.f;
  ident.retention = lawR.reflectivity;
  ion.yield = {0.f, 0.f, 0.f, 0.5f, 1.f};
  ion.energyMax = 100.f;
  ion.sourceQuantiles = {40.f, 80.f, 100.f};
  ion.retention = {1.f, 0.3f};
  ionNoCut = ion;
  ionNoCut.energyCut = false;
  bad.yield = {0.f, -1.f};

  if (!tracer.gatherEnergy(64, ones, none, 0.3f).empty())
    return fail("an energy gather before any apply must be refused");
  tracer.apply();
  if (tracer.getRayTraceInfo().error)
    return fail("apply");
  const std::vector<float> flux = tracer.getLocalData().getVectorData(0);
  const size_t n = points.size();

  for (GatherReflection kind : {GatherReflection::SPECULAR, GatherReflection::DIFFUSE}) {
    const std::vector<float> angular = tracer.gatherAngular(100, mixed, 0.2f, kind, 8);
    if (angular.size() != n || tracer.gatherEnergy(100, ones, mixed, 0.2f, kind, 8) != angular)
      return fail("an all-ones yield is gatherAngular");
    const vr_gather_spec s8 = Tracer::pathsSpec(nullptr, 0.8f, kind, 8), s1 = Tracer::pathsSpec(nullptr, 1.f, kind, 8);
    std::vector<int64_t> a1, a2, b1, b2;
    if (!tracer.gatherEnergySums(s8, mixed, twice, 0, 1, 64, a1, a2) || !tracer.gatherAngularSums(s8, mixed, 0, 1, 64, b1, b2))
      return fail("gatherEnergySums");
    for (size_t i = 0; i < n; ++i)
      if (a1[i] != 2 * b1[i])
        return fail("Y_E = 2 doubles the sums");
    if (!tracer.gatherEnergySums(s1, none, ident, 0, 1, 64, a1, a2) || !tracer.gatherAngularSums(s1, lawR, 0, 1, 64, b1, b2) || a1 != b1 ||
        a2 != b2)
      return fail("retention R under the yield {0, 1} is the reflectivity law R");
    if (!tracer.gatherEnergySums(s8, none, ion, 0, 2, 128, a1, a2) || !tracer.gatherEnergySums(s8, none, ionNoCut, 0, 2, 128, b1, b2) ||
        a1 != b1 || a2 != b2)
      return fail("the cut changes no sum");
  }

  const std::vector<float> want = tracer.gatherEnergy(256, ion, mixed, 0.2f, GatherReflection::SPECULAR, 8);
  if (want.size() != n)
    return fail("gatherEnergy");
  std::printf("ion");
  for (float v : want)
    std::printf(" %a", (double)v);
  std::printf("\n");
  const auto fine = tracer.gatherEnergyAdaptive(0.f, ion, mixed, 0.2f, GatherReflection::SPECULAR, 8, 64, 256);
  if (fine.flux != want || fine.samplesUsed != std::vector<unsigned>(n, 256u))
    return fail("target 0 is gatherEnergy(maxSamples)");

  Tracer::GatherEnergy noYield = ion, zeroMax = ion, big = twice;
  noYield.yield.clear();
  zeroMax.energyMax = 0.f;
  if (!tracer.gatherEnergy(64, bad, none, 0.2f).empty() || !tracer.gatherEnergy(64, noYield, none, 0.2f).empty() ||
      !tracer.gatherEnergy(64, zeroMax, none, 0.2f).empty() || !tracer.gatherEnergy(1u << 22, big, none, 0.2f).empty())
    return fail("a negative yield, a missing yield, energyMax 0, samples x wbound above 2^22 must be refused");
  if (tracer.getLocalData().getVectorData(0) != flux)
    return fail("the flux after an energy gather");

  float *dOut = nullptr;
  if (hipMalloc((void **)&dOut, n * 4) != hipSuccess)
    return fail("hipMalloc");
  const unsigned third = (unsigned)n / 3;
  const vr_gather_spec s2 = Tracer::pathsSpec(nullptr, 1.f - 0.2f, GatherReflection::SPECULAR, 8);
  std::vector<float> got(n);
  if (!tracer.gatherEnergyDevice(s2, mixed, ion, 0, third, 256, dOut) ||
      !tracer.gatherEnergyDevice(s2, mixed, ion, third, (unsigned)n - third, 256, dOut + third) || hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(got.data(), dOut, n * 4, hipMemcpyDeviceToHost) != hipSuccess)
    return fail("gatherEnergyDevice");
  if (std::memcmp(got.data(), want.data(), n * 4))
    return fail("the device form over two ranges differs from the host form");
  if (tracer.gatherEnergyDevice(s2, mixed, ion, 0, (unsigned)n, 256, got.data()))
    return fail("a host pointer must be refused");
  (void)hipFree(dOut);
  std::printf("facade gather energy ok\n");
  return 0;
}
