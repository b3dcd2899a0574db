// vr_gather_angular.cpp — vr_gather_angular* / vr_debug_gather_angular_path: the path gather weighed by tabulated angular
// laws — source radiance, reflectivity by incidence, yield by the starting angle (include/viennaray_amd.h has the
// definition; vr_gather.hip the kernels — the gather's own sample loop in its PATH 3 instantiations — vr_gather.hpp the
// look-up, the normalisation and the weight rule).  The laws are checked and normalised here, on the host, before anything
// is touched; the calls themselves are those of vr_gather_paths.cpp and vr_gather_adaptive.cpp, which take the laws as
// one more argument: one implementation for the entry points with and without them.
#include <cmath>
#include <cstring>
#include <string>

#include "vr_context.hpp"
#include "vr_gather.hpp"

namespace vr {

static_assert(sizeof(GatherLawSet::table) == 3 * GATHER_LAW_MAX * sizeof(float), "GatherLawSet holds the device table");

int gather_laws_refusal(vr_context *c, const char *api, const vr_gather_laws *laws, float cosinePower, uint32_t samples,
                        GatherLawSet &set) {
  set = GatherLawSet{};
  set.wbound = (double)gather_g(cosinePower, c->geo.D);
  if (!laws)
    return VR_OK;
  const std::string name = api;
  const float *tables[3] = {laws->sourceLaw, laws->reflectivityLaw, laws->yieldLaw};
  const uint32_t counts[3] = {laws->sourceCount, laws->reflectivityCount, laws->yieldCount};
  static const char *const names[3] = {"sourceLaw", "reflectivityLaw", "yieldLaw"};
  static const char *const ranges[3] = {"finite and >= 0", "in [0, 1]", "finite and >= 0"};
  for (int w = 0; w < 3; ++w) {
    if (!tables[w])
      continue;
    if (!gather_law_count_ok(counts[w]))
      return fail(c, VR_E_INVALID, (name + ": " + names[w] + " must have 2 .. 256 entries").c_str());
    const uint32_t bad = gather_law_first_bad(w, tables[w], counts[w]);
    if (bad != counts[w])
      return fail(c, VR_E_INVALID,
                  (name + ": " + names[w] + "[" + std::to_string(bad) + "] is not " + ranges[w] + " (the lowest such index)").c_str());
    set.any = true;
    set.count[w] = counts[w];
    std::memcpy(set.table + (size_t)w * GATHER_LAW_MAX, tables[w], (size_t)counts[w] * 4);
  }
  const int D = c->geo.D;
  double wbound = (double)gather_g(cosinePower, D);
  if (tables[GATHER_LAW_SOURCE]) {
    const float *L = tables[GATHER_LAW_SOURCE];
    const uint32_t M = counts[GATHER_LAW_SOURCE];
    if (cosinePower != 1.f)
      return fail(c, VR_E_INVALID, (name + ": a sourceLaw takes the place of the power cosine: cosinePower must be 1").c_str());
    if (!(gather_law_max(L, M) > 0.f) || !(gather_law_norm(L, M, D) > 0.))
      return fail(c, VR_E_INVALID, (name + ": sourceLaw must not be 0 everywhere").c_str());
    set.gL = gather_law_g(L, M, D);
    wbound = (double)set.gL * (double)gather_law_max(L, M);
  }
  if (tables[GATHER_LAW_YIELD])
    wbound *= (double)gather_law_max(tables[GATHER_LAW_YIELD], counts[GATHER_LAW_YIELD]);
  // (the int64 sum of a primitive holds samples x the largest weight: gather_wmax)
  if (!(wbound <= (double)gather_wmax(samples)))
    return fail(c, VR_E_INVALID,
                (name + ": samples x wbound must stay below 2^22, wbound = (g_L max L or g) max Y (the int64 sums' range)").c_str());
  set.wbound = wbound;
  return VR_OK;
}

int gather_laws_args(vr_context *c, bool &waited, const GatherLawSet &set, GatherArgs &a) {
  if (!set.any)
    return VR_OK;
  VR_TRY(map_grow(c, c->dGatherLaws, 3 * GATHER_LAW_MAX, waited));
  VR_HIP(c, launch_gather_laws(set.table, c->dGatherLaws.p, c->stream));
  a.laws = c->dGatherLaws.p;
  for (int w = 0; w < 3; ++w)
    a.lawCount[w] = set.count[w];
  a.gL = set.gL;
  return VR_OK;
}

// what an angular entry point asks of its spec, and the laws it hands on: a caller's NULL means "no law", which still is
// an angular call
static const vr_gather_laws NO_LAWS = {nullptr, 0u, nullptr, 0u, nullptr, 0u};
static int angular_spec(vr_context *c, const char *api, const vr_gather_spec *s, const vr_gather_laws *&laws) {
  const std::string name = api;
  if (!s)
    return fail(c, VR_E_INVALID, (name + ": spec must not be null").c_str());
  if (s->paths != 1u || s->mode != VR_GATHER_NORMAL || s->emission)
    return fail(c, VR_E_INVALID, (name + ": spec.paths must be 1, spec.mode VR_GATHER_NORMAL and spec.emission NULL").c_str());
  if (!laws)
    laws = &NO_LAWS;
  return VR_OK;
}

} // namespace vr

using namespace vr;

extern "C" {

int vr_gather_angular_device(vr_context *c, const vr_gather_spec *s, const vr_gather_laws *laws, uint32_t primFirst,
                             uint32_t primCount, uint32_t samples, float *out, void *stream) {
  if (!c)
    return VR_E_INVALID;
  const char *api = "vr_gather_angular_device";
  VR_TRY(angular_spec(c, api, s, laws));
  return paths_call_device(c, api, laws, primFirst, primCount, samples, s->cosinePower, s->reflection, s->maxBounces, s->reflectivity,
                           s->reflectivityScalar, out, stream);
}

int vr_gather_angular(vr_context *c, const vr_gather_spec *s, const vr_gather_laws *laws, uint32_t primFirst, uint32_t primCount,
                      uint32_t samples, float *out) {
  if (!c)
    return VR_E_INVALID;
  const char *api = "vr_gather_angular";
  VR_TRY(angular_spec(c, api, s, laws));
  return paths_call_host(c, api, laws, primFirst, primCount, samples, s->cosinePower, s->reflection, s->maxBounces, s->reflectivity,
                         s->reflectivityScalar, out);
}

int vr_gather_angular_sums_device(vr_context *c, const vr_gather_spec *s, const vr_gather_laws *laws, uint32_t primFirst,
                                  uint32_t primCount, uint32_t chunkFirst, uint32_t chunks, uint32_t budget, int64_t *sum,
                                  int64_t *sumSq, void *stream) {
  if (!c)
    return VR_E_INVALID;
  const char *api = "vr_gather_angular_sums_device";
  VR_TRY(angular_spec(c, api, s, laws));
  return sums_call_device(c, api, s, laws, primFirst, primCount, chunkFirst, chunks, budget, sum, sumSq, stream);
}

int vr_gather_angular_sums(vr_context *c, const vr_gather_spec *s, const vr_gather_laws *laws, uint32_t primFirst,
                           uint32_t primCount, uint32_t chunkFirst, uint32_t chunks, uint32_t budget, int64_t *sum,
                           int64_t *sumSq) {
  if (!c)
    return VR_E_INVALID;
  const char *api = "vr_gather_angular_sums";
  VR_TRY(angular_spec(c, api, s, laws));
  return sums_call_host(c, api, s, laws, primFirst, primCount, chunkFirst, chunks, budget, sum, sumSq);
}

int vr_gather_angular_adaptive_device(vr_context *c, const vr_gather_spec *s, const vr_gather_laws *laws, uint32_t primFirst,
                                      uint32_t primCount, uint32_t minSamples, uint32_t maxSamples, float relTarget,
                                      float absTarget, float *flux, float *stdErr, uint32_t *samplesUsed,
                                      vr_gather_adaptive_info *info, void *stream) {
  if (!c)
    return VR_E_INVALID;
  const char *api = "vr_gather_angular_adaptive_device";
  VR_TRY(angular_spec(c, api, s, laws));
  return adaptive_call_device(c, api, s, laws, primFirst, primCount, minSamples, maxSamples, relTarget, absTarget, flux, stdErr,
                              samplesUsed, info, stream);
}

int vr_gather_angular_adaptive(vr_context *c, const vr_gather_spec *s, const vr_gather_laws *laws, uint32_t primFirst,
                               uint32_t primCount, uint32_t minSamples, uint32_t maxSamples, float relTarget, float absTarget,
                               float *flux, float *stdErr, uint32_t *samplesUsed, vr_gather_adaptive_info *info) {
  if (!c)
    return VR_E_INVALID;
  const char *api = "vr_gather_angular_adaptive";
  VR_TRY(angular_spec(c, api, s, laws));
  return adaptive_call_host(c, api, s, laws, primFirst, primCount, minSamples, maxSamples, relTarget, absTarget, flux, stdErr,
                            samplesUsed, info);
}

int vr_debug_gather_angular_path(vr_context *c, const vr_gather_spec *s, const vr_gather_laws *laws, uint32_t prim, uint32_t sample,
                                 uint32_t maxVertices, uint32_t *vertexIds, float *vertexData, uint32_t *numVertices, uint32_t *end,
                                 float *finalDirection3, float *throughput, float *weight) {
  if (!c)
    return VR_E_INVALID;
  const char *api = "vr_debug_gather_angular_path";
  VR_TRY(angular_spec(c, api, s, laws));
  return paths_call_debug(c, api, laws, prim, sample, s->cosinePower, s->reflection, s->maxBounces, s->reflectivity,
                          s->reflectivityScalar, maxVertices, vertexIds, vertexData, numVertices, end, finalDirection3, throughput,
                          weight);
}

} // extern "C"
