// Trace::gatherSpeciesAdaptive / gatherSpeciesAdaptiveDevice: several species to a target error each, along one set of
// traced paths, through the façade, on the folded sheet of facade_gather_species.cpp.  Checks: every row of flux, stdErr and
// samplesUsed is vr_gather_angular_adaptive of that species under its own targets word for word, the info is made of the
// single calls' infos, the device form over two ranges is the host form, a missing target, five species and a negative
// target come back empty, a gather leaves the flux of the apply as it was.  Prints the flux rows and "facade gather species
// adaptive ok" when everything holds.
#include <hip/hip_runtime_api.h>

#include <rayBoundary.hpp>
#include <rayParticle.hpp>
#include <rayTraceDisk.hpp>

#include <algorithm>
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
  const std::vector<float> rel = {0.05f, 0.1f, 0.2f, 0.02f}, abs = {0.f, 0.f, 0.05f, 0.f};
  constexpr unsigned MINS = 64, MAXS = 512, MB = 8;

  if (!tracer.gatherSpeciesAdaptive(rel, species, GatherReflection::SPECULAR, MB, MINS, MAXS, abs).flux.empty())
    return fail("an adaptive species gather before any apply must be refused");
  tracer.apply();
  if (tracer.getRayTraceInfo().error)
    return fail("apply");
  const std::vector<float> flux = tracer.getLocalData().getVectorData(0);

  for (GatherReflection kind : {GatherReflection::SPECULAR, GatherReflection::DIFFUSE}) {
    const auto res = tracer.gatherSpeciesAdaptive(rel, species, kind, MB, MINS, MAXS, abs);
    if (res.flux.size() != 4 * n || res.stdErr.size() != 4 * n || res.samplesUsed.size() != 4 * n)
      return fail("gatherSpeciesAdaptive");
    std::vector<vr_gather_spec> specs;
    std::vector<vr_gather_laws> laws;
    Tracer::speciesPods(species, kind, MB, specs, laws);
    uint32_t rounds = 0;
    uint64_t sumTotal = 0, walked = 0;
    for (size_t s = 0; s < 4; ++s) {
      std::vector<float> f(n), e(n);
      std::vector<uint32_t> u(n);
      vr_gather_adaptive_info one{};
      if (vr_gather_angular_adaptive(tracer.getContext(), &specs[s], &laws[s], 0u, (uint32_t)n, MINS, MAXS, rel[s], abs[s], f.data(),
                                     e.data(), u.data(), &one) != VR_OK)
        return fail("vr_gather_angular_adaptive of one species");
      if (std::memcmp(f.data(), res.flux.data() + s * n, n * 4) || std::memcmp(e.data(), res.stdErr.data() + s * n, n * 4) ||
          std::memcmp(u.data(), res.samplesUsed.data() + s * n, n * 4))
        return fail("a row differs from gatherAngularAdaptive of its species");
      if (one.unconverged != res.info.unconverged[s] || one.totalSamples != res.info.totalSamples[s])
        return fail("unconverged / totalSamples of a species differ from its own call's");
      rounds = std::max(rounds, one.rounds);
      sumTotal += one.totalSamples;
    }
    for (size_t i = 0; i < n; ++i) {
      unsigned m = 0;
      for (size_t s = 0; s < 4; ++s)
        m = std::max(m, res.samplesUsed[s * n + i]);
      walked += m;
    }
    if (res.info.rounds != rounds || res.info.walkedSamples != walked || !(walked < sumTotal))
      return fail("rounds / walkedSamples");
    if (kind == GatherReflection::SPECULAR) {
      std::printf("rows");
      for (float v : res.flux)
        std::printf(" %a", (double)v);
      std::printf("\n");
    }
  }

  // refusals: a target short, five species, a negative target of species 2 — and the flux of the apply is what it was
  std::vector<Tracer::GatherSpecies> five(5);
  std::vector<float> negative = rel;
  negative[2] = -0.1f;
  if (!tracer.gatherSpeciesAdaptive({0.1f, 0.1f}, species).flux.empty() ||
      !tracer.gatherSpeciesAdaptive({0.1f, 0.1f, 0.1f, 0.1f, 0.1f}, five).flux.empty() ||
      !tracer.gatherSpeciesAdaptive(negative, species, GatherReflection::SPECULAR, MB, MINS, MAXS).flux.empty() ||
      !tracer.gatherSpeciesAdaptive(rel, species, GatherReflection::SPECULAR, MB, 100, 400).flux.empty())
    return fail("a missing target, five species, a negative target and minSamples 100 must be refused");
  if (tracer.getLocalData().getVectorData(0) != flux)
    return fail("the flux after an adaptive species gather");

  // the device form over two ranges (scalars only: the tables of a device call are device memory), stdErr left out
  std::vector<Tracer::GatherSpecies> three = {species[0], species[2], species[3]};
  const std::vector<float> rel3 = {rel[0], rel[2], rel[3]}, abs3 = {abs[0], abs[2], abs[3]};
  const auto want = tracer.gatherSpeciesAdaptive(rel3, three, GatherReflection::SPECULAR, MB, MINS, MAXS, abs3);
  if (want.flux.size() != 3 * n)
    return fail("gatherSpeciesAdaptive of three");
  std::vector<vr_gather_spec> specs;
  std::vector<vr_gather_laws> laws;
  Tracer::speciesPods(three, GatherReflection::SPECULAR, MB, specs, laws);
  float *dFlux = nullptr;
  uint32_t *dUsed = nullptr;
  const unsigned head = 37u, tailCount = (unsigned)n - head;
  if (hipMalloc((void **)&dFlux, 3 * n * 4) != hipSuccess || hipMalloc((void **)&dUsed, 3 * n * 4) != hipSuccess)
    return fail("hipMalloc");
  std::vector<float> a(3 * (size_t)head), b(3 * (size_t)tailCount);
  std::vector<uint32_t> ua(3 * (size_t)head), ub(3 * (size_t)tailCount);
  vr_gather_species_adaptive_info ia{}, ib{};
  if (!tracer.gatherSpeciesAdaptiveDevice(specs, laws.data(), 0, head, MINS, MAXS, rel3.data(), abs3.data(), dFlux, nullptr, dUsed, ia) ||
      hipDeviceSynchronize() != hipSuccess || hipMemcpy(a.data(), dFlux, a.size() * 4, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(ua.data(), dUsed, ua.size() * 4, hipMemcpyDeviceToHost) != hipSuccess ||
      !tracer.gatherSpeciesAdaptiveDevice(specs, laws.data(), head, tailCount, MINS, MAXS, rel3.data(), abs3.data(), dFlux, nullptr, dUsed,
                                          ib) ||
      hipDeviceSynchronize() != hipSuccess || hipMemcpy(b.data(), dFlux, b.size() * 4, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(ub.data(), dUsed, ub.size() * 4, hipMemcpyDeviceToHost) != hipSuccess)
    return fail("gatherSpeciesAdaptiveDevice");
  for (size_t s = 0; s < 3; ++s)
    if (std::memcmp(a.data() + s * head, want.flux.data() + s * n, head * 4) ||
        std::memcmp(b.data() + s * tailCount, want.flux.data() + s * n + head, tailCount * 4) ||
        std::memcmp(ua.data() + s * head, want.samplesUsed.data() + s * n, head * 4) ||
        std::memcmp(ub.data() + s * tailCount, want.samplesUsed.data() + s * n + head, tailCount * 4))
      return fail("the device form over two ranges differs from the host form");
  for (size_t s = 0; s < 3; ++s)
    if (ia.totalSamples[s] + ib.totalSamples[s] != want.info.totalSamples[s] ||
        ia.unconverged[s] + ib.unconverged[s] != want.info.unconverged[s])
      return fail("the infos of two ranges do not add up to the whole range's");
  if (ia.walkedSamples + ib.walkedSamples != want.info.walkedSamples)
    return fail("walkedSamples of two ranges");
  if (tracer.gatherSpeciesAdaptiveDevice(specs, laws.data(), 0, (unsigned)n, MINS, MAXS, rel3.data(), abs3.data(), a.data(), nullptr,
                                         nullptr, ia))
    return fail("a host pointer must be refused");
  (void)hipFree(dFlux);
  (void)hipFree(dUsed);
  std::printf("facade gather species adaptive ok\n");
  return 0;
}
