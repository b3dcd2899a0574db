// The façade's DataLog (rayUtil.hpp:49-63 and Trace::getDataLog(), rayTrace.hpp, of the reference): a stateful device model
// with a log_data hook fills the log the caller sized; every apply() ADDS to what is there (the reference merges its
// per-thread logs into the Trace's and never clears them, rayTraceKernel.hpp:75-82, 345); an empty log stays empty.
// Prints "facade data log ok" when everything holds.
#include <rayParticle.hpp>
#include <rayTraceDisk.hpp>

#include <cstdio>
#include <string>
#include <vector>

using namespace viennaray;

static const char *kModel = R"(
struct VrUserModel : ModelDiffuse {
  static constexpr bool kNeedsFull = true;
  static constexpr int kStateWords = 1;
  static constexpr int kLogRows = 2;
  __device__ static void init(const ModelCtx &, RayState &s, Rng &rng, unsigned &t2) { s.v[0] = 2.f * canon_f32(rng_next(rng, t2)); }
  template <class Log> __device__ static void log_data(const ModelCtx &, const RayState &s, Log &&log) {
    log(0, (int)(s.v[0] * 32.f), 1.f);
    log(1, (int)(s.v[0] * 32.f), s.v[0]);
  }
  template <int D>
  __device__ static Reflection surface_reflection(const ModelCtx &, RayState &, float w, const V3 &rayDir, const V3 &n,
                                                  unsigned, int, float base, Rng &rng, unsigned &t2) {
    Reflection r{base, rayDir};
    if (w - w * base > 0.f)
      r.dir = reflection_diffuse<D>(n, rng, t2);
    return r;
  }
  template <class Credit>
  __device__ static void collide(const ModelCtx &, const RayState &, float w, const V3 &, const V3 &, unsigned, int,
                                 Credit &&credit) {
    credit(0, w);
  }
};
)";

static int fail(const char *what) {
  std::printf("FAILED: %s\n", what);
  return 1;
}

static double rowSum(const std::vector<float> &row) {
  double s = 0;
  for (float v : row)
    s += v;
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
  const unsigned rays = 50000;

  TraceDisk<float, 3> tracer;
  tracer.setGeometry(points, normals, 1.f);
  tracer.setNumberOfRaysFixed(rays);
  tracer.setUseRandomSeeds(false);
  const int kind = tracer.registerParticleModel("ionLog", kModel, 1, 1);
  if (kind < 0)
    return fail("the model did not register");
  auto particle = std::make_unique<UserModelParticle<float, 3>>(kind, 0.5f, std::vector<std::string>{"flux"});
  tracer.setParticleType(particle);

  // an empty log stays empty
  tracer.apply();
  if (tracer.getRayTraceInfo().error || !tracer.getDataLog().data.empty())
    return fail("an empty log must stay empty");

  DataLog<float> &log = tracer.getDataLog();
  log.data.assign(2, std::vector<float>(64, 0.f));
  tracer.apply();
  if (tracer.getRayTraceInfo().error)
    return fail("first apply with a log");
  const std::vector<float> first0 = log.data[0], first1 = log.data[1];
  if (rowSum(first0) != (double)rays)
    return fail("row 0 counts every ray once");
  if (!(rowSum(first1) > 0.9 * rays && rowSum(first1) < 1.1 * rays)) // (E uniform in [0, 2): mean 1)
    return fail("row 1 sums the energies");

  tracer.apply(); // (another run number: other rays)
  if (tracer.getRayTraceInfo().error)
    return fail("second apply with a log");
  if (rowSum(log.data[0]) != 2.0 * rays)
    return fail("the second apply's log is ADDED to the first");
  bool grew = true, differs = false;
  for (int b = 0; b < 64; ++b) {
    grew = grew && log.data[0][b] >= first0[b] && log.data[1][b] >= first1[b];
    differs = differs || log.data[0][b] != 2.f * first0[b];
  }
  if (!grew || !differs)
    return fail("every bin grows, by the second apply's own histogram");

  // a particle that logs nothing leaves a sized log alone
  auto diffuse = std::make_unique<DiffuseParticle<float, 3>>(0.5f, "flux");
  tracer.setParticleType(diffuse);
  const std::vector<float> before = log.data[0];
  tracer.apply();
  if (tracer.getRayTraceInfo().error || log.data[0] != before)
    return fail("a particle without a hook leaves the log as it is");

  // the host virtual stays a no-op
  DataLog<float> host;
  host.data.assign(1, std::vector<float>(4, 0.f));
  particle->logData(host);
  if (rowSum(host.data[0]) != 0.0)
    return fail("UserModelParticle::logData is a host no-op");
  std::printf("facade data log ok\n");
  return 0;
}
