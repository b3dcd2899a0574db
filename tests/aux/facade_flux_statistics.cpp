// Trace::setCalculateFluxError / getHitCounts / getFluxRelativeError / getFluxAbsoluteError / getFluxErrorDevice on the
// C++ façade.  Without a HIP device every member is called on a trace that has no context: nothing may crash, the
// getters return empty vectors, and the program prints "facade flux statistics ok (no device)".  With one, a small
// trench of disks is traced with a reflecting and with an absorbing particle:
//   - the getters are refused (empty) while statistics are off, and before an apply;
//   - the flux with statistics on has the bits of the flux with statistics off;
//   - sigma follows its definition from hits and flux where every credit is a unit weight (absorbing particle);
//   - the device getter returns the host getter's floats.
// Prints "facade flux statistics ok".
#include <hip/hip_runtime_api.h>

#include <rayParticle.hpp>
#include <rayTraceDisk.hpp>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace viennaray;

static int fail(const char *what) {
  std::printf("FAILED: %s\n", what);
  return 1;
}

template <class Tracer> static bool run(Tracer &tracer, float sticking, std::vector<float> &flux) {
  auto particle = std::make_unique<DiffuseParticle<float, 3>>(sticking, "flux");
  tracer.setParticleType(particle);
  vr_set_run_number(tracer.getContext(), 1);
  tracer.apply();
  if (tracer.getRayTraceInfo().error)
    return false;
  flux = tracer.getLocalData().getVectorData(0);
  return true;
}

int main() {
  constexpr int N = 24;
  constexpr unsigned RAYS = 40000;
  std::vector<Vec3D<float>> points, normals;
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) {
      const float slope = 1.4f * std::cos(0.7f * i), len = std::sqrt(slope * slope + 1.f);
      points.push_back({(float)i, (float)j, 2.f * std::sin(0.7f * i)});
      normals.push_back({-slope / len, 0.f, 1.f / len});
    }
  const size_t n = points.size();

  TraceDisk<float, 3> tracer;
  if (!tracer.getContext()) {
    // no device: every member on a trace without a context
    tracer.setCalculateFluxError(true);
    if (!tracer.getHitCounts().empty() || !tracer.getFluxRelativeError().empty() || !tracer.getFluxAbsoluteError(0).empty() ||
        tracer.getFluxErrorDevice(nullptr))
      return fail("getters of a trace without a device must return nothing");
    std::printf("facade flux statistics ok (no device)\n");
    return 0;
  }
  tracer.setGeometry(points, normals, 1.f);
  tracer.setNumberOfRaysFixed(RAYS);
  tracer.setUseRandomSeeds(false);

  std::vector<float> off, on, offAbsorb, onAbsorb;
  if (!run(tracer, 0.3f, off))
    return fail("the apply with statistics off");
  if (!tracer.getHitCounts().empty() || !tracer.getFluxRelativeError().empty())
    return fail("the getters must be refused while statistics are off");
  tracer.setCalculateFluxError(true);
  if (!tracer.getHitCounts().empty())
    return fail("the getters must be refused before an apply with statistics on");
  if (!run(tracer, 0.3f, on))
    return fail("the apply with statistics on");
  if (on.size() != n || std::memcmp(on.data(), off.data(), n * 4) != 0)
    return fail("statistics on changed the flux");
  const std::vector<uint64_t> hits = tracer.getHitCounts();
  const std::vector<float> rel = tracer.getFluxRelativeError(), abs = tracer.getFluxAbsoluteError();
  if (hits.size() != n || rel.size() != n || abs.size() != n)
    return fail("the getters' sizes");
  uint64_t total = 0;
  for (size_t i = 0; i < n; ++i) {
    total += hits[i];
    if ((hits[i] == 0) != (on[i] == 0.f) || (hits[i] == 0 ? !std::isinf(rel[i]) : !(rel[i] > 0.f && rel[i] < 1.f)))
      return fail("hit counts, flux and relative error disagree");
    if (hits[i] && std::fabs(abs[i] / on[i] - rel[i]) > 1e-5f * rel[i])
      return fail("relative error is not sigma / S1");
  }
  if (total < tracer.getRayTraceInfo().geometryHits)
    return fail("fewer credits than surface hits");
  // the device getter: the host getter's floats
  float *dOut = nullptr;
  if (hipMalloc((void **)&dOut, n * 4) != hipSuccess)
    return fail("hipMalloc");
  std::vector<float> back(n);
  for (int relative = 0; relative <= 1; ++relative) {
    if (!tracer.getFluxErrorDevice(dOut, 0, relative != 0) || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(back.data(), dOut, n * 4, hipMemcpyDeviceToHost) != hipSuccess)
      return fail("getFluxErrorDevice");
    if (std::memcmp(back.data(), (relative ? rel : abs).data(), n * 4) != 0)
      return fail("the device getter differs from the host getter");
  }
  (void)hipFree(dOut);
  // an absorbing particle: unit weights, hits = flux and sigma^2 = S1 - S1^2 / N
  tracer.setCalculateFluxError(false);
  if (!run(tracer, 1.f, offAbsorb))
    return fail("the absorbing apply with statistics off");
  tracer.setCalculateFluxError(true);
  if (!run(tracer, 1.f, onAbsorb) || std::memcmp(onAbsorb.data(), offAbsorb.data(), n * 4) != 0)
    return fail("statistics on changed the absorbing flux");
  const std::vector<uint64_t> hitsAbsorb = tracer.getHitCounts();
  const std::vector<float> absAbsorb = tracer.getFluxAbsoluteError();
  for (size_t i = 0; i < n; ++i) {
    if ((float)hitsAbsorb[i] != onAbsorb[i])
      return fail("absorbing particle: hits differ from the flux");
    const double s1 = (double)hitsAbsorb[i], want = std::sqrt(std::fmax(s1 - s1 * s1 / RAYS, 0.0));
    if (std::fabs((double)absAbsorb[i] - want) > 1e-6 * want)
      return fail("absorbing particle: sigma is not sqrt(S1 - S1^2 / N)");
  }
  std::printf("facade flux statistics ok\n");
  return 0;
}
