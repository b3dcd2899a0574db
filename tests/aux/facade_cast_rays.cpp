// Trace::castRays / castRaysDevice: closest-hit queries for the caller's rays.  A flat sheet of disks is traced once;
// a vertical ray at a disk's centre must come back with that disk, its distance and its point, a ray pointing up with a
// miss, and the device form must agree with the host form word for word.  Prints "facade cast rays ok" when everything holds.
#include <hip/hip_runtime_api.h>

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
  constexpr int N = 24;
  std::vector<std::array<float, 3>> points, normals;
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) {
      points.push_back({(float)i, (float)j, 0.f});
      normals.push_back({0.f, 0.f, 1.f});
    }

  TraceDisk<float, 3> tracer;
  tracer.setGeometry(points, normals, 1.f);
  tracer.setNumberOfRaysFixed(20000);
  tracer.setUseRandomSeeds(false);
  auto particle = std::make_unique<DiffuseParticle<float, 3>>(0.3f, "flux");
  tracer.setParticleType(particle);

  CastResult<float> res;
  const std::vector<Vec3D<float>> oneOrg = {{11.f, 13.f, 5.f}}, oneDir = {{0.f, 0.f, -1.f}};
  if (tracer.castRays(oneOrg, oneDir, res))
    return fail("a cast before any apply must be refused");

  tracer.apply();
  if (tracer.getRayTraceInfo().error)
    return fail("apply");
  const std::vector<float> flux = tracer.getLocalData().getVectorData(0);

  // the disk at (11, 13) is primitive 11 * N + 13; ray 1 points up; ray 2 is oblique and follows the side walls
  const std::vector<Vec3D<float>> org = {{11.f, 13.f, 5.f}, {11.f, 13.f, 5.f}, {3.25f, 4.5f, 2.f}, {20.f, 2.f, 0.5f}};
  const std::vector<Vec3D<float>> dir = {{0.f, 0.f, -1.f}, {0.f, 0.f, 1.f}, {0.3f, -0.2f, -1.f}, {1.f, 0.25f, -0.01f}};
  const size_t m = org.size();
  if (!tracer.castRays(org, dir, res))
    return fail("castRays");
  if (res.primIDs.size() != m || res.distances.size() != m || res.hitPoints.size() != m || res.boundaryHits.size() != m)
    return fail("castRays: sizes");
  if (res.primIDs[0] != 11 * N + 13 || res.distances[0] != 5.f || res.boundaryHits[0] != 0u ||
      res.hitPoints[0] != Vec3D<float>{11.f, 13.f, 0.f})
    return fail("the vertical ray at a disk's centre");
  if (res.primIDs[1] != VR_CAST_MISS || !std::isinf(res.distances[1]) || !std::isnan(res.hitPoints[1][0]))
    return fail("the ray pointing up");
  if (res.primIDs[2] < 0 || res.primIDs[3] < 0 || res.boundaryHits[3] == 0u)
    return fail("the oblique rays");
  CastResult<float> near, plain;
  if (!tracer.castRays(org, dir, near, 4.f) || near.primIDs[0] != VR_CAST_MISS || !std::isinf(near.distances[0]))
    return fail("tmax below the distance");
  if (!tracer.castRays(org, dir, plain, std::numeric_limits<float>::infinity(), false) || plain.primIDs[3] != VR_CAST_WALL ||
      plain.primIDs[0] != res.primIDs[0])
    return fail("followBoundaries off");
  if (tracer.getLocalData().getVectorData(0) != flux)
    return fail("the flux after a cast");

  float *dOrg = nullptr, *dDir = nullptr, *dDist = nullptr, *dHit = nullptr;
  int32_t *dPrim = nullptr;
  uint32_t *dBh = nullptr;
  if (hipMalloc((void **)&dOrg, m * 12) != hipSuccess || hipMalloc((void **)&dDir, m * 12) != hipSuccess ||
      hipMalloc((void **)&dDist, m * 4) != hipSuccess || hipMalloc((void **)&dHit, m * 12) != hipSuccess ||
      hipMalloc((void **)&dPrim, m * 4) != hipSuccess || hipMalloc((void **)&dBh, m * 4) != hipSuccess)
    return fail("hipMalloc");
  if (hipMemcpy(dOrg, org.data(), m * 12, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dDir, dir.data(), m * 12, hipMemcpyHostToDevice) != hipSuccess)
    return fail("hipMemcpy");
  std::vector<int32_t> prim(m);
  std::vector<float> dist(m);
  std::vector<Vec3D<float>> hit(m);
  std::vector<uint32_t> bh(m);
  if (!tracer.castRaysDevice(dOrg, dDir, m, 3, std::numeric_limits<float>::infinity(), VR_CAST_FOLLOW_BOUNDARIES, dPrim, dDist,
                             dHit, dBh) ||
      hipDeviceSynchronize() != hipSuccess || hipMemcpy(prim.data(), dPrim, m * 4, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(dist.data(), dDist, m * 4, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(hit.data(), dHit, m * 12, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(bh.data(), dBh, m * 4, hipMemcpyDeviceToHost) != hipSuccess)
    return fail("castRaysDevice");
  for (size_t i = 0; i < m; ++i)
    if (prim[i] != res.primIDs[i] || std::memcmp(&dist[i], &res.distances[i], 4) != 0 || bh[i] != res.boundaryHits[i] ||
        std::memcmp(&hit[i], &res.hitPoints[i], 12) != 0)
      return fail("the device form differs from the host form");
  // the optional outputs may be left out
  if (!tracer.castRaysDevice(dOrg, dDir, m, 3, 100.f, 0u, dPrim, dDist) || hipDeviceSynchronize() != hipSuccess)
    return fail("castRaysDevice without the optional outputs");
  // a host pointer is refused
  if (tracer.castRaysDevice(&org[0][0], dDir, m, 3, 100.f, 0u, dPrim, dDist))
    return fail("a host pointer must be refused");

  (void)hipFree(dOrg);
  (void)hipFree(dDir);
  (void)hipFree(dDist);
  (void)hipFree(dHit);
  (void)hipFree(dPrim);
  (void)hipFree(dBh);
  std::printf("facade cast rays ok\n");
  return 0;
}
