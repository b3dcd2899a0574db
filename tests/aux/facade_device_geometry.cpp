// TraceDisk::setGeometryDevice / Trace::getFluxDevice: a surface that lives in device memory goes in where it is, and
// the flux comes back to device memory.  The same rippled plane is traced twice — through the host setGeometry and
// through the device entry points — and every flux value must have the same bits.
// Prints "facade device geometry ok" when everything holds.
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

template <class Tracer> static void configure(Tracer &tracer) {
  tracer.setNumberOfRaysFixed(50000);
  tracer.setUseRandomSeeds(false);
  auto particle = std::make_unique<DiffuseParticle<float, 3>>(0.3f, "flux");
  tracer.setParticleType(particle);
}

int main() {
  constexpr int N = 24;
  std::vector<Vec3D<float>> points, normals;
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) {
      points.push_back({(float)i, (float)j, 0.5f * std::sin(0.7f * i) * std::cos(0.4f * j)});
      normals.push_back({0.f, 0.f, 1.f});
    }
  const size_t n = points.size();

  TraceDisk<float, 3> host;
  host.setGeometry(points, normals, 1.f);
  configure(host);
  host.apply();
  if (host.getRayTraceInfo().error)
    return fail("the host-geometry apply");
  std::vector<float> want = host.getLocalData().getVectorData(0);
  std::vector<float> wantNorm = want;
  host.normalizeFlux(wantNorm, NormalizationType::SOURCE);
  host.smoothFlux(wantNorm, 1);

  std::vector<float> flatP(3 * n), flatN(3 * n);
  for (size_t i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) {
      flatP[3 * i + k] = points[i][k];
      flatN[3 * i + k] = normals[i][k];
    }
  float *dP = nullptr, *dN = nullptr, *dFlux = nullptr;
  if (hipMalloc((void **)&dP, flatP.size() * 4) != hipSuccess || hipMalloc((void **)&dN, flatN.size() * 4) != hipSuccess ||
      hipMalloc((void **)&dFlux, n * 4) != hipSuccess)
    return fail("hipMalloc");
  if (hipMemcpy(dP, flatP.data(), flatP.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dN, flatN.data(), flatN.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
    return fail("hipMemcpy");

  TraceDisk<float, 3> dev;
  dev.setGeometryDevice(dP, dN, n, 3, 1.f);
  // copy-on-set: the caller's rows may go at once
  if (hipMemset(dP, 0, flatP.size() * 4) != hipSuccess || hipMemset(dN, 0, flatN.size() * 4) != hipSuccess)
    return fail("hipMemset");
  configure(dev);
  dev.apply();
  if (dev.getRayTraceInfo().error)
    return fail("the device-geometry apply");
  if (dev.getLocalData().getVectorData(0) != want)
    return fail("device geometry: the flux differs from the host geometry's");

  std::vector<float> got(n);
  if (!dev.getFluxDevice(dFlux) || hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(got.data(), dFlux, n * 4, hipMemcpyDeviceToHost) != hipSuccess)
    return fail("getFluxDevice (raw)");
  if (std::memcmp(got.data(), want.data(), n * 4) != 0)
    return fail("getFluxDevice (raw) differs from getLocalData()");
  if (!dev.getFluxDevice(dFlux, 0, NormalizationType::SOURCE, 1) || hipDeviceSynchronize() != hipSuccess ||
      hipMemcpy(got.data(), dFlux, n * 4, hipMemcpyDeviceToHost) != hipSuccess)
    return fail("getFluxDevice (normalised, smoothed)");
  if (std::memcmp(got.data(), wantNorm.data(), n * 4) != 0)
    return fail("getFluxDevice (normalised, smoothed) differs from normalizeFlux + smoothFlux");

  // a host pointer is refused and the geometry stays
  dev.setGeometryDevice(flatP.data(), flatN.data(), n, 3, 1.f);
  if (!dev.getRayTraceInfo().error)
    return fail("a host pointer must be refused");

  (void)hipFree(dP);
  (void)hipFree(dN);
  (void)hipFree(dFlux);
  std::printf("facade device geometry ok\n");
  return 0;
}
