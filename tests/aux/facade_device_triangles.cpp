// TraceTriangle::setGeometryDevice: a triangle mesh that lives in device memory goes in where it is.  The same rippled
// grid mesh is traced twice — through setGeometry(TriangleMesh) and through the device entry point — and every flux value
// must have the same bits.
// Prints "facade device triangles ok" when everything holds.
#include <hip/hip_runtime_api.h>

#include <rayParticle.hpp>
#include <rayTraceTriangle.hpp>

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
  constexpr int N = 20; // (N + 1)^2 vertices, 2 N^2 = 800 triangles: four tiles of 256, the last one partial
  TriangleMesh mesh;
  mesh.gridDelta = 1.f;
  for (int i = 0; i <= N; ++i)
    for (int j = 0; j <= N; ++j)
      mesh.nodes.push_back({(float)i, (float)j, 0.5f * std::sin(0.7f * i) * std::cos(0.4f * j)});
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) {
      const unsigned a = i * (N + 1) + j, b = a + (N + 1), c = a + 1, d = b + 1;
      mesh.triangles.push_back({a, b, c});
      mesh.triangles.push_back({c, b, d});
    }
  const size_t nv = mesh.nodes.size(), nt = mesh.triangles.size();

  TraceTriangle<float, 3> host;
  host.setGeometry(mesh);
  configure(host);
  host.apply();
  if (host.getRayTraceInfo().error)
    return fail("the host-geometry apply");
  const std::vector<float> want = host.getLocalData().getVectorData(0);
  bool any = false;
  for (float f : want)
    any = any || f != 0.f;
  if (!any)
    return fail("the host-geometry flux is all zero");

  std::vector<float> flatV(3 * nv);
  std::vector<unsigned> flatT(3 * nt);
  for (size_t i = 0; i < nv; ++i)
    for (int k = 0; k < 3; ++k)
      flatV[3 * i + k] = mesh.nodes[i][k];
  for (size_t i = 0; i < nt; ++i)
    for (int k = 0; k < 3; ++k)
      flatT[3 * i + k] = mesh.triangles[i][k];
  float *dV = nullptr;
  unsigned *dT = nullptr;
  if (hipMalloc((void **)&dV, flatV.size() * 4) != hipSuccess || hipMalloc((void **)&dT, flatT.size() * 4) != hipSuccess)
    return fail("hipMalloc");
  if (hipMemcpy(dV, flatV.data(), flatV.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dT, flatT.data(), flatT.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
    return fail("hipMemcpy");

  TraceTriangle<float, 3> dev;
  dev.setGeometryDevice(dV, nv, dT, nt, mesh.gridDelta);
  // copy-on-set: the caller's buffers may go at once
  if (hipMemset(dV, 0, flatV.size() * 4) != hipSuccess || hipMemset(dT, 0, flatT.size() * 4) != hipSuccess)
    return fail("hipMemset");
  configure(dev);
  dev.apply();
  if (dev.getRayTraceInfo().error)
    return fail("the device-geometry apply");
  const std::vector<float> got = dev.getLocalData().getVectorData(0);
  if (got.size() != want.size() || std::memcmp(got.data(), want.data(), want.size() * 4) != 0)
    return fail("device geometry: the flux differs from the host geometry's");

  // a host pointer is refused and the geometry stays
  dev.setGeometryDevice(flatV.data(), nv, flatT.data(), nt, mesh.gridDelta);
  if (!dev.getRayTraceInfo().error)
    return fail("a host pointer must be refused");

  (void)hipFree(dV);
  (void)hipFree(dT);
  std::printf("facade device triangles ok\n");
  return 0;
}
