// Trace::gatherFlux / gatherFluxDevice: per-primitive direct flux by rays cast from the surface.  A flat sheet of disks
// between periodic walls sees the whole source: every value is exactly 1 under a power-1 source, whatever the sample
// count; the device form agrees with the host form word for word; a gather leaves the flux of the apply as it was.
// Prints "facade gather flux ok" when everything holds.
#include <hip/hip_runtime_api.h>

#include <rayBoundary.hpp>
#include <rayParticle.hpp>
#include <rayTraceDisk.hpp>

#include <array>
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
      points.push_back({(float)i, (float)j, 0.f});
      normals.push_back({0.f, 0.f, 1.f});
    }

  TraceDisk<float, 3> tracer;
  tracer.setGeometry(points, normals, 1.f);
  BoundaryCondition bcs[3] = {BoundaryCondition::PERIODIC_BOUNDARY, BoundaryCondition::PERIODIC_BOUNDARY,
                              BoundaryCondition::PERIODIC_BOUNDARY};
  tracer.setBoundaryConditions(bcs);
  tracer.setNumberOfRaysFixed(20000);
  tracer.setUseRandomSeeds(false);
  auto particle = std::make_unique<DiffuseParticle<float, 3>>(0.3f, "flux");
  tracer.setParticleType(particle);

  if (!tracer.gatherFlux(64).empty())
    return fail("a gather before any apply must be refused");

  tracer.apply();
  if (tracer.getRayTraceInfo().error)
    return fail("apply");
  const std::vector<float> flux = tracer.getLocalData().getVectorData(0);
  const size_t n = points.size();

  const std::vector<float> one = tracer.gatherFlux(100);
  if (one.size() != n)
    return fail("gatherFlux: size");
  for (float v : one)
    if (v != 1.f)
      return fail("an unoccluded flat surface under a power-1 source is exactly 1");
  const std::vector<float> zeros(n, 0.f);
  const std::vector<float> power = tracer.gatherFlux(64, 8.f), source = tracer.gatherFlux(64, 8.f, GatherMode::SOURCE),
                           withTable = tracer.gatherFlux(64, 8.f, GatherMode::NORMAL, &zeros);
  if (power.size() != n || source.size() != n || withTable != power)
    return fail("gatherFlux with a source power, with SOURCE sampling, with an emission table of zeros");
  for (float v : source)
    if (v != 1.f) // (facing the source: m . w / c = 1 for every sample)
      return fail("SOURCE sampling on a surface facing the source is exactly 1");
  if (!tracer.gatherFlux(0).empty() || !tracer.gatherFlux(64, 1.f, GatherMode::SOURCE).empty() ||
      !tracer.gatherFlux(64, 8.f, GatherMode::SOURCE, &zeros).empty())
    return fail("no samples, SOURCE with power 1, SOURCE with a table must be refused");
  if (tracer.getLocalData().getVectorData(0) != flux)
    return fail("the flux after a gather");

  float *dOut = nullptr;
  if (hipMalloc((void **)&dOut, n * 4) != hipSuccess)
    return fail("hipMalloc");
  std::vector<float> got(n);
  const unsigned third = (unsigned)n / 3;
  if (!tracer.gatherFluxDevice(0, third, 64, 8.f, GatherMode::NORMAL, nullptr, dOut) ||
      !tracer.gatherFluxDevice(third, (unsigned)n - third, 64, 8.f, GatherMode::NORMAL, nullptr, dOut + third) ||
      hipDeviceSynchronize() != hipSuccess || hipMemcpy(got.data(), dOut, n * 4, hipMemcpyDeviceToHost) != hipSuccess)
    return fail("gatherFluxDevice");
  if (std::memcmp(got.data(), power.data(), n * 4) != 0)
    return fail("the device form over two ranges differs from the host form");
  if (tracer.gatherFluxDevice(0, (unsigned)n, 64, 1.f, GatherMode::NORMAL, nullptr, got.data()))
    return fail("a host pointer must be refused");
  (void)hipFree(dOut);
  std::printf("facade gather flux ok\n");
  return 0;
}
