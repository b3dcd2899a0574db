// Trace::solveRadiosity / solveRadiosityDevice / radiosityLinks: the steady-state flux of a diffusely re-emitting species
// from a recorded link table.  argv[1]: a disk cloud, one line "x y z nx ny nz" of hex floats per disk (gridDelta 1,
// walls REFLECTIVE / PERIODIC / REFLECTIVE, seed 7).  Checks the refusals and the forms against each other, then prints
// "flux <iterations> <residual bits>" and one line of eight hex digits per primitive — solveRadiosity(256, 0.25) — for the
// test to compare with the Python call bit for bit, and "facade radiosity ok" when everything holds.
#include <hip/hip_runtime_api.h>

#include <rayBoundary.hpp>
#include <rayParticle.hpp>
#include <rayTraceDisk.hpp>

#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace viennaray;

static int fail(const char *what) {
  std::printf("FAILED: %s\n", what);
  return 1;
}

int main(int argc, char **argv) {
  if (argc < 2)
    return fail("usage: facade_radiosity <disks>");
  std::vector<std::array<float, 3>> points, normals;
  if (FILE *f = std::fopen(argv[1], "r")) {
    char w[6][64];
    while (std::fscanf(f, "%63s %63s %63s %63s %63s %63s", w[0], w[1], w[2], w[3], w[4], w[5]) == 6) {
      points.push_back({std::strtof(w[0], nullptr), std::strtof(w[1], nullptr), std::strtof(w[2], nullptr)});
      normals.push_back({std::strtof(w[3], nullptr), std::strtof(w[4], nullptr), std::strtof(w[5], nullptr)});
    }
    std::fclose(f);
  }
  const size_t n = points.size();
  if (n == 0)
    return fail("no disks read");

  TraceDisk<float, 3> tracer;
  tracer.setGeometry(points, normals, 1.f);
  BoundaryCondition bcs[3] = {BoundaryCondition::REFLECTIVE_BOUNDARY, BoundaryCondition::PERIODIC_BOUNDARY,
                              BoundaryCondition::REFLECTIVE_BOUNDARY};
  tracer.setBoundaryConditions(bcs);
  tracer.setNumberOfRaysFixed(1000);
  tracer.setRngSeed(7);
  auto particle = std::make_unique<DiffuseParticle<float, 3>>(1.f, "flux");
  tracer.setParticleType(particle);

  if (!tracer.solveRadiosity(64, 0.5f).empty())
    return fail("a solve before any apply must be refused");
  tracer.apply();
  if (tracer.getRayTraceInfo().error)
    return fail("apply");
  const std::vector<float> flux = tracer.getLocalData().getVectorData(0);

  if (tracer.radiosityLinkBytes(256) < (uint64_t)n * 256 * 4 + n * 8)
    return fail("radiosityLinkBytes");
  // maxIterations = 0 is the direct flux: the gather's bits
  Trace<float, 3>::RadiosityInfo info;
  const std::vector<float> direct = tracer.solveRadiosity(256, 0.25f, 1.f, 1e-4f, 0, &info), gathered = tracer.gatherFlux(256);
  if (direct.size() != n || direct != gathered || info.iterations != 0 || info.residual != 0.f)
    return fail("solveRadiosity with maxIterations = 0 against gatherFlux");
  const std::vector<float> solved = tracer.solveRadiosity(256, 0.25f, 1.f, 1e-4f, 1000, &info);
  if (solved.size() != n || info.iterations == 0 || info.iterations >= 1000 || !(info.residual <= 1e-4f))
    return fail("solveRadiosity");
  bool grew = false;
  for (size_t i = 0; i < n; ++i) {
    if (solved[i] < direct[i])
      return fail("re-emission cannot lower a flux");
    grew = grew || solved[i] > direct[i];
  }
  if (!grew)
    return fail("re-emission raises the flux somewhere in a trench");
  // a table of sticking values, all alike: the scalar's bits
  const std::vector<float> table(n, 0.25f);
  Trace<float, 3>::RadiosityInfo info2;
  if (tracer.solveRadiosity(256, table, 1.f, 1e-4f, 1000, &info2) != solved || info2.iterations != info.iterations)
    return fail("per-primitive sticking");
  // refusals: sticking outside [0, 1], a negative tolerance, a table of the wrong size
  if (!tracer.solveRadiosity(256, 1.5f).empty() || !tracer.solveRadiosity(256, -0.5f).empty() ||
      !tracer.solveRadiosity(256, 0.25f, 1.f, -1.f).empty() || !tracer.solveRadiosity(256, std::vector<float>(n - 1, 0.25f)).empty() ||
      !tracer.solveRadiosity(0, 0.25f).empty())
    return fail("sticking outside [0, 1], a negative tolerance, a short table, no samples must be refused");
  if (tracer.getLocalData().getVectorData(0) != flux)
    return fail("the flux after a solve");

  // the device form on the resident table
  float *dOut = nullptr, *dRho = nullptr;
  if (hipMalloc((void **)&dOut, n * 4) != hipSuccess || hipMalloc((void **)&dRho, n * 4) != hipSuccess)
    return fail("hipMalloc");
  const std::vector<float> rho(n, 0.75f);
  std::vector<float> got(n);
  Trace<float, 3>::RadiosityInfo info3;
  if (hipMemcpy(dRho, rho.data(), n * 4, hipMemcpyHostToDevice) != hipSuccess ||
      !tracer.solveRadiosityDevice(dRho, 0.f, 1e-4f, 1000, dOut, &info3) || hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(got.data(), dOut, n * 4, hipMemcpyDeviceToHost) != hipSuccess)
    return fail("solveRadiosityDevice");
  if (std::memcmp(got.data(), solved.data(), n * 4) != 0 || info3.iterations != info.iterations)
    return fail("the device form differs from the host form");
  if (!tracer.solveRadiosityDevice(nullptr, 0.75f, 1e-4f, 1000, dOut) || hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(got.data(), dOut, n * 4, hipMemcpyDeviceToHost) != hipSuccess || std::memcmp(got.data(), solved.data(), n * 4) != 0)
    return fail("the device form with a scalar");
  if (tracer.solveRadiosityDevice(nullptr, 0.75f, 1e-4f, 1000, got.data()))
    return fail("a host pointer must be refused");
  tracer.freeRadiosityLinks();
  if (tracer.solveRadiosityDevice(nullptr, 0.75f, 1e-4f, 1000, dOut))
    return fail("the device form without a table must be refused");
  if (!tracer.radiosityLinks(256) || !tracer.solveRadiosityDevice(nullptr, 0.75f, 1e-4f, 1000, dOut))
    return fail("radiosityLinks, then the device form");
  (void)hipFree(dOut);
  (void)hipFree(dRho);

  uint32_t rbits;
  std::memcpy(&rbits, &info.residual, 4);
  std::printf("flux %u %08x\n", info.iterations, rbits);
  for (float v : solved) {
    uint32_t b;
    std::memcpy(&b, &v, 4);
    std::printf("%08x\n", b);
  }
  std::printf("facade radiosity ok\n");
  return 0;
}
