// Trace::setGlobalDataDevice / setMaterialIdsDevice / setSurfaceSourceDevice: the inputs of a time step that already live
// in device memory go in where they are.
//   1. a device-set global vector survives apply() calls around a borrowed TracingData that holds other values, until
//      setGlobalData(TracingData &) is called again;
//   2. one time step — disks, coverages, pass 1, flux, surface source weighted by that flux, pass 2, flux — with
//      hipMalloc'd buffers at every interface against the host setters: every float must have the same bits.
// Prints "facade device inputs ok" when everything holds.
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
  auto particle = std::make_unique<CoverageStickingParticle<float, 3>>(0.6f, "flux", 0);
  tracer.setParticleType(particle);
}

template <class Tracer> static bool run(Tracer &tracer, unsigned runNumber, std::vector<float> &flux) {
  vr_set_run_number(tracer.getContext(), runNumber);
  tracer.apply();
  if (tracer.getRayTraceInfo().error)
    return false;
  flux = tracer.getLocalData().getVectorData(0);
  return true;
}

static bool same(const std::vector<float> &a, const std::vector<float> &b) {
  return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * 4) == 0;
}

template <class T> static T *upload(const std::vector<T> &h) {
  T *d = nullptr;
  if (hipMalloc((void **)&d, h.size() * sizeof(T)) != hipSuccess ||
      hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess)
    return nullptr;
  return d;
}

int main() {
  constexpr int N = 24;
  std::vector<Vec3D<float>> points, normals;
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) {
      // grooves two cells deep with the normals of the height field: a reflected ray meets the slope opposite, so the
      // sticking (the coverage) shows in the flux
      const float slope = 1.4f * std::cos(0.7f * i), len = std::sqrt(slope * slope + 1.f);
      points.push_back({(float)i, (float)j, 2.f * std::sin(0.7f * i)});
      normals.push_back({-slope / len, 0.f, 1.f / len});
    }
  const size_t n = points.size();
  std::vector<float> cov(n), other(n), flatP(3 * n), flatN(3 * n);
  std::vector<int32_t> ids(n);
  for (size_t i = 0; i < n; ++i) {
    cov[i] = 0.05f + 0.9f * (float)((i * 37) % 101) / 101.f;
    other[i] = 0.9f - 0.8f * (float)((i * 11) % 53) / 53.f;
    ids[i] = (int32_t)(i % 3);
    for (int k = 0; k < 3; ++k) {
      flatP[3 * i + k] = points[i][k];
      flatN[3 * i + k] = normals[i][k];
    }
  }
  float *dCov = upload(cov), *dP = upload(flatP), *dN = upload(flatN), *dFlux = nullptr;
  int32_t *dIds = upload(ids);
  if (!dCov || !dP || !dN || !dIds || hipMalloc((void **)&dFlux, n * 4) != hipSuccess)
    return fail("hipMalloc / hipMemcpy");

  // ---- 1. a device-set vector and a borrowed TracingData --------------------------------------------------------
  TracingData<float> wantData, otherData;
  wantData.setNumberOfVectorData(2);
  wantData.setVectorData(0, cov, "coverage");
  wantData.setVectorData(1, other, "other");
  otherData.setNumberOfVectorData(2);
  otherData.setVectorData(0, other, "coverage"); // (other values at the index the device owns)
  otherData.setVectorData(1, cov, "other");
  std::vector<float> want, wantOther, got;
  {
    TraceDisk<float, 3> host;
    host.setGeometry(points, normals, 1.f);
    configure(host);
    host.setGlobalData(wantData);
    if (!run(host, 1, want))
      return fail("the host apply");
    host.setGlobalData(otherData);
    if (!run(host, 1, wantOther))
      return fail("the host apply with the other data");
    if (same(want, wantOther))
      return fail("the coverage must matter: the two host applies gave the same flux");
  }
  {
    TraceDisk<float, 3> dev;
    dev.setGeometry(points, normals, 1.f);
    configure(dev);
    dev.setGlobalData(otherData);
    dev.setGlobalDataDevice(0, dCov, n);
    for (int k = 0; k < 3; ++k) {
      otherData.getVectorData(1)[k] += 0.01f; // (the borrowed data changes between the applies, as it may)
      if (!run(dev, 1, got))
        return fail("an apply with a device-set vector");
      if (!same(got, want))
        return fail("the device-set vector 0 did not survive an apply around the borrowed TracingData");
    }
    for (int k = 0; k < 3; ++k)
      otherData.getVectorData(1)[k] -= 0.03f;
    dev.setGlobalData(otherData); // the host data wins again
    if (!run(dev, 1, got) || !same(got, wantOther))
      return fail("setGlobalData(TracingData &) after a device set must win again");
    dev.setGlobalDataDevice(0, flatP.data(), n); // a host pointer is refused
    if (!dev.getRayTraceInfo().error)
      return fail("a host pointer must be refused");
  }

  // ---- 2. one time step, host arrays against device buffers ---------------------------------------------------------
  std::vector<float> h1, h2, d1, d2;
  const float area = 123.5f, offset = 1e-4f;
  {
    TraceDisk<float, 3> host;
    host.setGeometry(points, normals, 1.f);
    host.setMaterialIds(ids);
    configure(host);
    host.setGlobalData(wantData);
    if (!run(host, 1, h1))
      return fail("host: pass 1");
    host.setSurfaceSource(points, normals, h1, area, offset); // the weights: the first pass's flux
    host.setNumberOfRaysPerPoint(20);
    if (!run(host, 2, h2))
      return fail("host: pass 2");
  }
  {
    TraceDisk<float, 3> dev;
    dev.setGeometryDevice(dP, dN, n, 3, 1.f);
    dev.setMaterialIdsDevice(dIds, n);
    configure(dev);
    dev.setGlobalDataDevice(0, dCov, n);
    if (hipMemset(dCov, 0, n * 4) != hipSuccess || hipMemset(dIds, 0, n * 4) != hipSuccess) // copy-on-set
      return fail("hipMemset");
    if (!run(dev, 1, d1))
      return fail("device: pass 1");
    if (!dev.getFluxDevice(dFlux))
      return fail("getFluxDevice");
    dev.setSurfaceSourceDevice(dP, dN, dFlux, n, 3, area, offset);
    if (dev.getRayTraceInfo().error)
      return fail("setSurfaceSourceDevice");
    dev.setNumberOfRaysPerPoint(20);
    if (!run(dev, 2, d2))
      return fail("device: pass 2");
    // a refused table (a negative weight) leaves the source in place
    std::vector<float> bad = h1;
    bad[n / 2] = -1.f;
    float *dBad = upload(bad);
    if (!dBad)
      return fail("hipMalloc");
    dev.setSurfaceSourceDevice(dP, dN, dBad, n, 3, area, offset);
    if (!dev.getRayTraceInfo().error)
      return fail("a negative weight must be refused");
    (void)hipFree(dBad);
  }
  if (!same(h1, d1))
    return fail("pass 1 differs between host and device inputs");
  if (!same(h2, d2))
    return fail("pass 2 differs between host and device inputs");
  bool any = false;
  for (float v : h2)
    any = any || v != 0.f;
  if (!any)
    return fail("pass 2 traced nothing");

  (void)hipFree(dCov);
  (void)hipFree(dP);
  (void)hipFree(dN);
  (void)hipFree(dIds);
  (void)hipFree(dFlux);
  std::printf("facade device inputs ok\n");
  return 0;
}
