// A user Source as device code through the C++ façade: registerSourceModel + setSourceModel + apply().  The source is the
// "Beam" of tests/test_source_models.py — origin uniform on the source face of the bounding box, direction
// normalize(a (2 r - 1), b (2 r - 1), posNeg) — with a ray count of its own.  Prints the flux checksum (the sum of the
// floats' bit patterns: exact and independent of the order), which the Python test compares with its own, and
// "facade source model ok" when everything holds.
#include <rayParticle.hpp>
#include <rayTraceDisk.hpp>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace viennaray;

static const char *kBeam = R"(
struct VrUserSource {
  static constexpr bool kHasWeight = false;
  template <int D, class Draw>
  __device__ static void sample(const SourceCtx &s, unsigned long long, Draw &&draw, V3 &org, V3 &dir, float &) {
    const float r1 = canon_f32(draw()), r2 = canon_f32(draw());
    org = mk(0.f, 0.f, 0.f);
    setc(org, s.rayDir, s.srcCoord);
    setc(org, s.firstDir, s.bbLo[s.firstDir] + (s.bbHi[s.firstDir] - s.bbLo[s.firstDir]) * r1);
    if (D == 3)
      setc(org, s.secondDir, s.bbLo[s.secondDir] + (s.bbHi[s.secondDir] - s.bbLo[s.secondDir]) * r2);
    const float r3 = canon_f32(draw()), r4 = canon_f32(draw());
    dir = mk(0.f, 0.f, 0.f);
    setc(dir, s.firstDir, s.params[0] * (2.f * r3 - 1.f));
    setc(dir, s.secondDir, D == 3 ? s.params[1] * (2.f * r4 - 1.f) : 0.f);
    setc(dir, s.rayDir, s.posNeg);
    vnormalize(dir);
  }
};
)";

static int fail(const char *what) {
  std::printf("FAILED: %s\n", what);
  return 1;
}

static unsigned long long checksum(const std::vector<float> &flux) {
  unsigned long long s = 0;
  for (float v : flux) {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    s += u;
  }
  return s;
}

int main() {
  constexpr int N = 24;
  std::vector<Vec3D<float>> points, normals;
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) {
      points.push_back({(float)i, (float)j, 0.f});
      normals.push_back({0.f, 0.f, 1.f});
    }
  const size_t rays = 4096;

  TraceDisk<float, 3> tracer;
  tracer.setGeometry(points, normals, 1.f);
  tracer.setRngSeed(4711);
  auto particle = std::make_unique<DiffuseParticle<float, 3>>(0.1f, "flux");
  tracer.setParticleType(particle);

  if (tracer.registerSourceModel("broken", "struct VrUserSource { no_such_type x; };") >= 0)
    return fail("a text that does not compile must not register");
  const int id = tracer.registerSourceModel("beam", kBeam);
  if (id < 0)
    return fail("the source model did not register");
  tracer.setSourceModel(id, {0.3f, 0.2f}, {}, rays);
  tracer.apply();
  if (tracer.getRayTraceInfo().error)
    return fail("apply with the source model");
  if (tracer.getRayTraceInfo().numRays != rays)
    return fail("the source's own ray count");
  const std::vector<float> flux = tracer.getLocalData().getVectorData(0);
  const unsigned long long sum = checksum(flux);

  // the source stays in force: the next apply (the run number moved on: other rays) counts the same
  tracer.apply();
  if (tracer.getRayTraceInfo().error || tracer.getRayTraceInfo().numRays != rays)
    return fail("second apply");
  // ... until SourceRandom takes its place again
  tracer.setSourceModel(-1);
  tracer.setNumberOfRaysFixed(rays);
  tracer.apply();
  if (tracer.getRayTraceInfo().error || checksum(tracer.getLocalData().getVectorData(0)) == sum)
    return fail("back to SourceRandom");

  std::printf("checksum %llu\n", sum);
  std::printf("facade source model ok\n");
  return 0;
}
