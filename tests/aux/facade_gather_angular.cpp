// Trace::gatherAngular / gatherAngularDevice / gatherAngularAdaptive / gatherAngularSums / debugGatherAngularPath: the path
// gather with angular laws through the façade, on the folded sheet of facade_gather_paths.cpp.  Checks: no law and all-ones
// laws are gatherPaths word for word, R = 0.5 at reflectivity 0.8 is gatherPaths at 0.4, Y = 2 doubles the int64 sums, the
// device form over two ranges is the host form, the adaptive call at target 0 is the fixed-K call at maxSamples, one path's
// weight is its throughput times the yield, refusals come back empty, a gather leaves the flux of the apply as it was.
// Prints "facade gather angular ok" when everything holds.
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

  Tracer::GatherLaws none, ones, half, twice, mixed, bad;
  ones.source.assign(2, 1.f);
  ones.reflectivity.assign(256, 1.f);
  ones.yield.assign(7, 1.f);
  half.reflectivity.assign(5, 0.5f);
  twice.yield.assign(3, 2.f);
  mixed.source = {0.f, 0.125f, 1.f};
  mixed.reflectivity = {1.f, 0.8f, 0.6f, 0.4f, 0.2f};
  mixed.yield = {0.5f, 3.f};
  bad.reflectivity = {0.5f, 1.5f};

  if (!tracer.gatherAngular(64, none, 0.3f).empty())
    return fail("an angular gather before any apply must be refused");
  tracer.apply();
  if (tracer.getRayTraceInfo().error)
    return fail("apply");
  const std::vector<float> flux = tracer.getLocalData().getVectorData(0);
  const size_t n = points.size();

  for (GatherReflection kind : {GatherReflection::SPECULAR, GatherReflection::DIFFUSE}) {
    const std::vector<float> paths = tracer.gatherPaths(64, 0.2f, kind, 8);
    if (paths.size() != n || tracer.gatherAngular(64, none, 0.2f, kind, 8) != paths)
      return fail("no law is gatherPaths");
    if (tracer.gatherAngular(64, ones, 0.2f, kind, 8) != paths)
      return fail("all-ones laws are gatherPaths");
    // (1 - 0.2f) * 0.5f is the float the scalar 1 - 0.6f is not: compare through the spec's own reflectivity
    const vr_gather_spec s8 = Tracer::pathsSpec(nullptr, 0.8f, kind, 8), s4 = Tracer::pathsSpec(nullptr, 0.4f, kind, 8);
    std::vector<int64_t> a1, a2, b1, b2;
    if (!tracer.gatherAngularSums(s8, half, 0, 1, 64, a1, a2) || !tracer.gatherSums(s4, 0, 1, 64, b1, b2) || a1 != b1 || a2 != b2)
      return fail("R = 0.5 at reflectivity 0.8 is reflectivity 0.4");
    if (!tracer.gatherAngularSums(s8, twice, 0, 1, 64, a1, a2) || !tracer.gatherSums(s8, 0, 1, 64, b1, b2))
      return fail("gatherAngularSums");
    for (size_t i = 0; i < n; ++i)
      if (a1[i] != 2 * b1[i])
        return fail("Y = 2 doubles the sums");
  }

  const std::vector<float> want = tracer.gatherAngular(256, mixed, 0.2f, GatherReflection::SPECULAR, 8);
  if (want.size() != n)
    return fail("gatherAngular with three laws");
  std::printf("mixed");
  for (float v : want)
    std::printf(" %a", (double)v);
  std::printf("\n");
  const auto fine = tracer.gatherAngularAdaptive(0.f, mixed, 0.2f, GatherReflection::SPECULAR, 8, 64, 256);
  if (fine.flux != want || fine.samplesUsed != std::vector<unsigned>(n, 256u))
    return fail("target 0 is gatherAngular(maxSamples)");

  const vr_gather_spec spec = Tracer::pathsSpec(nullptr, 0.8f, GatherReflection::SPECULAR, 8);
  Tracer::GatherPathRecord rec;
  Tracer::GatherLaws yieldOnly;
  yieldOnly.yield = mixed.yield;
  if (!tracer.debugGatherAngularPath(spec, yieldOnly, 5, 3, 10, rec) || rec.numVertices < 1 || rec.ids[0] != 5u)
    return fail("debugGatherAngularPath");
  if (rec.end == VR_GATHER_END_MISS && rec.direction[2] > 0.f) {
    // mu0 from vertex 0: its normal (floats 6 .. 8) and its leaving direction (floats 9 .. 11); Y is linear over two nodes
    const float *v0 = rec.data.data();
    const float mu0 = std::fmin(std::fmax((v0[6] * v0[9] + v0[7] * v0[10]) + v0[8] * v0[11], 0.f), 1.f);
    const float slope = mu0 * (3.f - 0.5f);
    const float y = 0.5f + slope;
    if (rec.weight != rec.throughput * y)
      return fail("one path's weight is T Y(mu0)");
  }

  if (!tracer.gatherAngular(64, bad, 0.2f).empty() || !tracer.gatherAngular(64, mixed, 0.2f, GatherReflection::SPECULAR, 8, 2.f).empty() ||
      !tracer.gatherAngular(1u << 22, twice, 0.2f).empty())
    return fail("a reflectivity above 1, a source law with cosinePower 2, samples x wbound above 2^22 must be refused");
  if (tracer.getLocalData().getVectorData(0) != flux)
    return fail("the flux after an angular gather");

  float *dOut = nullptr;
  if (hipMalloc((void **)&dOut, n * 4) != hipSuccess)
    return fail("hipMalloc");
  const unsigned third = (unsigned)n / 3;
  const vr_gather_spec s2 = Tracer::pathsSpec(nullptr, 1.f - 0.2f, GatherReflection::SPECULAR, 8);
  std::vector<float> got(n);
  if (!tracer.gatherAngularDevice(s2, mixed, 0, third, 256, dOut) ||
      !tracer.gatherAngularDevice(s2, mixed, third, (unsigned)n - third, 256, dOut + third) || hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(got.data(), dOut, n * 4, hipMemcpyDeviceToHost) != hipSuccess)
    return fail("gatherAngularDevice");
  if (std::memcmp(got.data(), want.data(), n * 4))
    return fail("the device form over two ranges differs from the host form");
  if (tracer.gatherAngularDevice(s2, mixed, 0, (unsigned)n, 256, got.data()))
    return fail("a host pointer must be refused");
  vr_gather_adaptive_info info{};
  if (!tracer.gatherAngularAdaptiveDevice(s2, mixed, 0, (unsigned)n, 64, 256, 0.f, 0.f, dOut, nullptr, nullptr, info) ||
      hipDeviceSynchronize() != hipSuccess || hipMemcpy(got.data(), dOut, n * 4, hipMemcpyDeviceToHost) != hipSuccess ||
      std::memcmp(got.data(), want.data(), n * 4) || info.rounds != 3u)
    return fail("gatherAngularAdaptiveDevice");
  (void)hipFree(dOut);
  std::printf("facade gather angular ok\n");
  return 0;
}
