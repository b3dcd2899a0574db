// Trace::gatherSpecies / gatherSpeciesDevice / gatherSpeciesSums: several species along one set of traced paths through
// the façade, on the folded sheet of facade_gather_angular.cpp.  Checks: every row is gatherAngular of that species word
// for word (a scalar, a per-primitive table, laws, another cosinePower), the sums' rows are gatherAngularSums's, the device
// form over two ranges is the host form, five species, no species and a bad law come back empty, a gather leaves the flux
// of the apply as it was.  Prints "facade gather species ok" when everything holds.
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
  const size_t n = points.size();

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

  std::vector<Tracer::GatherSpecies> species(4);
  species[0].sticking = 0.2f;
  species[1].reflectivity.assign(n, 0.9f);
  for (size_t i = 0; i < n; i += 3)
    species[1].reflectivity[i] = 0.f; // a third of the sheet absorbs species 1 outright
  species[2].sticking = 0.f;
  species[2].laws.reflectivity = {1.f, 0.2f};
  species[2].laws.yield = {0.5f, 1.125f, 1.75f, 2.375f, 3.f};
  species[3].sticking = 0.4f;
  species[3].cosinePower = 8.f;

  if (!tracer.gatherSpecies(64, species).empty())
    return fail("a species gather before any apply must be refused");
  tracer.apply();
  if (tracer.getRayTraceInfo().error)
    return fail("apply");
  const std::vector<float> flux = tracer.getLocalData().getVectorData(0);

  for (GatherReflection kind : {GatherReflection::SPECULAR, GatherReflection::DIFFUSE}) {
    const std::vector<float> rows = tracer.gatherSpecies(100, species, kind, 8);
    if (rows.size() != 4 * n)
      return fail("gatherSpecies");
    std::vector<vr_gather_spec> specs;
    std::vector<vr_gather_laws> laws;
    Tracer::speciesPods(species, kind, 8, specs, laws);
    std::vector<int64_t> s1, s2, a1, a2;
    if (!tracer.gatherSpeciesSums(species, kind, 8, 0, 1, 128, s1, s2) || s1.size() != 4 * n || s2.size() != 4 * n)
      return fail("gatherSpeciesSums");
    for (size_t s = 0; s < 4; ++s) {
      std::vector<float> one(n);
      if (vr_gather_angular(tracer.getContext(), &specs[s], &laws[s], 0u, (uint32_t)n, 100u, one.data()) != VR_OK)
        return fail("vr_gather_angular of one species");
      if (std::memcmp(one.data(), rows.data() + s * n, n * 4))
        return fail("a row differs from gatherAngular of its species");
      if (!tracer.gatherAngularSums(specs[s], species[s].laws, 0, 1, 128, a1, a2))
        return fail("gatherAngularSums of one species");
      if (std::memcmp(a1.data(), s1.data() + s * n, n * 8) || std::memcmp(a2.data(), s2.data() + s * n, n * 8))
        return fail("a row of the sums differs from gatherAngularSums of its species");
    }
    if (kind == GatherReflection::SPECULAR) {
      if (!std::memcmp(rows.data(), rows.data() + n, n * 4))
        return fail("rows 0 and 1 must differ");
      std::printf("rows");
      for (float v : rows)
        std::printf(" %a", (double)v);
      std::printf("\n");
    }
  }

  // refusals: too many species, none, a bad law in species 1 — and the flux of the apply is what it was
  std::vector<Tracer::GatherSpecies> five(5), bad(species.begin(), species.begin() + 2);
  bad[1].laws.yield = {1.f, -2.f};
  if (!tracer.gatherSpecies(64, five).empty() || !tracer.gatherSpecies(64, {}).empty() || !tracer.gatherSpecies(64, bad).empty())
    return fail("five species, no species and a negative yield must be refused");
  if (tracer.getLocalData().getVectorData(0) != flux)
    return fail("the flux after a species gather");

  // the device form over two ranges (scalars only: the tables of a device call are device memory)
  std::vector<Tracer::GatherSpecies> three = {species[0], species[2], species[3]};
  const std::vector<float> want = tracer.gatherSpecies(64, three, GatherReflection::SPECULAR, 8);
  if (want.size() != 3 * n)
    return fail("gatherSpecies of three");
  std::vector<vr_gather_spec> specs;
  std::vector<vr_gather_laws> laws;
  Tracer::speciesPods(three, GatherReflection::SPECULAR, 8, specs, laws);
  float *dOut = nullptr;
  const unsigned head = 65u, tailCount = (unsigned)n - head;
  if (hipMalloc((void **)&dOut, 3 * n * 4) != hipSuccess)
    return fail("hipMalloc");
  std::vector<float> a(3 * (size_t)head), b(3 * (size_t)tailCount);
  if (!tracer.gatherSpeciesDevice(specs, laws.data(), 0, head, 64, dOut) || hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(a.data(), dOut, a.size() * 4, hipMemcpyDeviceToHost) != hipSuccess ||
      !tracer.gatherSpeciesDevice(specs, laws.data(), head, tailCount, 64, dOut) || hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(b.data(), dOut, b.size() * 4, hipMemcpyDeviceToHost) != hipSuccess)
    return fail("gatherSpeciesDevice");
  for (size_t s = 0; s < 3; ++s)
    if (std::memcmp(a.data() + s * head, want.data() + s * n, head * 4) ||
        std::memcmp(b.data() + s * tailCount, want.data() + s * n + head, tailCount * 4))
      return fail("the device form over two ranges differs from the host form");
  if (tracer.gatherSpeciesDevice(specs, laws.data(), 0, (unsigned)n, 64, a.data()))
    return fail("a host pointer must be refused");
  (void)hipFree(dOut);
  std::printf("facade gather species ok\n");
  return 0;
}
