// Trace::mapToPointsDevice / getFluxAtPointsDevice / mapToPoints: per-primitive values at the caller's points.  A flat
// sheet of disks is traced once; the values 0, 1, 2, ... mapped to the disks' own centres with radius 0 must come back as
// they are, from the host form and from the device form alike, and the flux at those centres must be the flux.
// Prints "facade map points ok" when everything holds.
#include <hip/hip_runtime_api.h>

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
  constexpr int N = 24;
  std::vector<std::array<float, 3>> points, normals;
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) {
      points.push_back({(float)i, (float)j, 0.f});
      normals.push_back({0.f, 0.f, 1.f});
    }
  const size_t n = points.size();

  TraceDisk<float, 3> tracer;
  tracer.setGeometry(points, normals, 1.f);
  tracer.setNumberOfRaysFixed(20000);
  tracer.setUseRandomSeeds(false);
  auto particle = std::make_unique<DiffuseParticle<float, 3>>(0.3f, "flux");
  tracer.setParticleType(particle);
  tracer.apply();
  if (tracer.getRayTraceInfo().error)
    return fail("apply");

  std::vector<float> values(n);
  for (size_t i = 0; i < n; ++i)
    values[i] = (float)i;
  const std::vector<float> host = tracer.mapToPoints(values, points, {}, 0.f);
  if (host != values)
    return fail("the host form at the own centres with radius 0");
  const std::vector<float> gated = tracer.mapToPoints(values, points, normals, 2.f);
  if (gated.size() != n)
    return fail("the host form with normals");

  float *dValues = nullptr, *dPoints = nullptr, *dOut = nullptr;
  if (hipMalloc((void **)&dValues, n * 4) != hipSuccess || hipMalloc((void **)&dPoints, n * 12) != hipSuccess ||
      hipMalloc((void **)&dOut, n * 4) != hipSuccess)
    return fail("hipMalloc");
  if (hipMemcpy(dValues, values.data(), n * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dPoints, points.data(), n * 12, hipMemcpyHostToDevice) != hipSuccess)
    return fail("hipMemcpy");
  std::vector<float> got(n);
  if (!tracer.mapToPointsDevice(dValues, dPoints, nullptr, n, 3, 0.f, dOut) || hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(got.data(), dOut, n * 4, hipMemcpyDeviceToHost) != hipSuccess || got != values)
    return fail("the device form at the own centres with radius 0");

  const std::vector<float> flux = tracer.getLocalData().getVectorData(0);
  if (!tracer.getFluxAtPointsDevice(dPoints, nullptr, n, 3, 0.f, dOut) || hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(got.data(), dOut, n * 4, hipMemcpyDeviceToHost) != hipSuccess ||
      std::memcmp(got.data(), flux.data(), n * 4) != 0)
    return fail("the raw flux at the own centres");
  if (!tracer.getFluxAtPointsDevice(dPoints, nullptr, n, 3, 0.f, dOut, 0, NormalizationType::SOURCE, 1))
    return fail("the normalised, smoothed flux at the own centres");

  // a host pointer is refused
  if (tracer.mapToPointsDevice(values.data(), dPoints, nullptr, n, 3, 0.f, dOut))
    return fail("a host pointer must be refused");

  (void)hipFree(dValues);
  (void)hipFree(dPoints);
  (void)hipFree(dOut);
  std::printf("facade map points ok\n");
  return 0;
}
