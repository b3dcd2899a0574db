// Trace::gatherPaths / gatherPathsDevice: multi-bounce flux by paths traced back from the surface.  A sheet of disks folded
// into V grooves (slopes +-1.5, period 8) between periodic walls, so that samples bounce; tests/test_gather_paths.py builds
// the same scene and compares the printed values bit for bit.  Checks here: maxBounces = 0 and sticking 1 are gatherFlux
// word for word, a per-primitive table of one value is the scalar's result, the device form over two ranges is the host
// form, refusals come back empty, a path gather leaves the flux of the apply as it was.
// Prints "specular <n hex floats>", "diffuse <n hex floats>" and "facade gather paths ok" when everything holds.
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
      const double s = k < 4 ? -1. : 1.; // the slope's sign: down to the groove's bottom at k = 4, up again
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

  if (!tracer.gatherPaths(64, 0.3f).empty())
    return fail("a path gather before any apply must be refused");
  tracer.apply();
  if (tracer.getRayTraceInfo().error)
    return fail("apply");
  const std::vector<float> flux = tracer.getLocalData().getVectorData(0);
  const size_t n = points.size();

  const std::vector<float> direct = tracer.gatherFlux(64);
  if (direct.size() != n)
    return fail("gatherFlux");
  for (GatherReflection r : {GatherReflection::SPECULAR, GatherReflection::DIFFUSE})
    if (tracer.gatherPaths(64, 0.3f, r, 0) != direct || tracer.gatherPaths(64, 1.f, r, 8) != direct)
      return fail("maxBounces 0 and sticking 1 are gatherFlux word for word");
  const std::vector<float> specular = tracer.gatherPaths(64, 0.3f, GatherReflection::SPECULAR, 8),
                           diffuse = tracer.gatherPaths(64, 0.3f, GatherReflection::DIFFUSE, 8);
  if (specular.size() != n || diffuse.size() != n)
    return fail("gatherPaths: size");
  bool more = false;
  for (size_t i = 0; i < n; ++i) {
    if (specular[i] < direct[i] || diffuse[i] < direct[i])
      return fail("reflections can only add to the direct flux");
    more = more || specular[i] > direct[i];
  }
  if (!more)
    return fail("no sample of the grooves bounced");
  if (tracer.gatherPaths(64, std::vector<float>(n, 0.3f), GatherReflection::SPECULAR, 8) != specular)
    return fail("a table of one value differs from the scalar");
  if (!tracer.gatherPaths(0, 0.3f).empty() || !tracer.gatherPaths(64, -0.5f).empty() || !tracer.gatherPaths(64, 1.5f).empty() ||
      !tracer.gatherPaths(64, 0.3f, GatherReflection::SPECULAR, 65536).empty() ||
      !tracer.gatherPaths(64, 0.3f, (GatherReflection)2).empty() || !tracer.gatherPaths(64, std::vector<float>(n - 1, 0.3f)).empty())
    return fail("no samples, a reflectivity outside [0, 1], too many bounces, an unknown reflection, a short table must be refused");
  if (tracer.getLocalData().getVectorData(0) != flux)
    return fail("the flux after a path gather");

  float *dOut = nullptr;
  if (hipMalloc((void **)&dOut, n * 4) != hipSuccess)
    return fail("hipMalloc");
  std::vector<float> got(n);
  const unsigned third = (unsigned)n / 3;
  const float rho = 1.f - 0.3f;
  if (!tracer.gatherPathsDevice(0, third, 64, 1.f, GatherReflection::DIFFUSE, 8, nullptr, rho, dOut) ||
      !tracer.gatherPathsDevice(third, (unsigned)n - third, 64, 1.f, GatherReflection::DIFFUSE, 8, nullptr, rho, dOut + third) ||
      hipDeviceSynchronize() != hipSuccess || hipMemcpy(got.data(), dOut, n * 4, hipMemcpyDeviceToHost) != hipSuccess)
    return fail("gatherPathsDevice");
  if (std::memcmp(got.data(), diffuse.data(), n * 4) != 0)
    return fail("the device form over two ranges differs from the host form");
  if (tracer.gatherPathsDevice(0, (unsigned)n, 64, 1.f, GatherReflection::SPECULAR, 8, nullptr, rho, got.data()))
    return fail("a host pointer must be refused");
  (void)hipFree(dOut);
  std::printf("specular");
  for (float v : specular)
    std::printf(" %a", v);
  std::printf("\ndiffuse");
  for (float v : diffuse)
    std::printf(" %a", v);
  std::printf("\nfacade gather paths ok\n");
  return 0;
}
