// vr_gather_energy.cpp — vr_gather_energy* / vr_debug_gather_energy_path: the angular gather with an ion's energy carried
// along every path — the energy at the source, the share kept at each reflection, a yield by the arrival energy
// (include/viennaray_amd.h has the definition; vr_gather_energy.hip the kernel, vr_gather.hpp the arithmetic).  The tables
// are checked here, on the host, before anything is touched; the calls themselves are those of vr_gather_paths.cpp and
// vr_gather_adaptive.cpp, which take the energy as one more argument and launch through gather_launch: one implementation
// for the entry points with and without it, and the existing ones launch exactly what they launched.
#include <cmath>
#include <cstring>
#include <string>

#include "vr_context.hpp"
#include "vr_gather.hpp"

static_assert(VR_GATHER_END_ENERGY == vr::GATHER_END_ENERGY, "vr_gather.hpp's constant is the header's");

namespace vr {

static_assert(sizeof(GatherEnergySet::table) == 3 * GATHER_LAW_MAX * sizeof(float), "GatherEnergySet holds the device table");

int gather_energy_refusal(vr_context *c, const char *api, const struct vr_gather_energy *energy, double wboundAngular, uint32_t samples,
                          GatherEnergySet &set) {
  set = GatherEnergySet{};
  if (!energy)
    return VR_OK;
  const std::string name = api;
  if (!energy->energyYield)
    return fail(c, VR_E_INVALID, (name + ": energyYield must not be null").c_str());
  const float *tables[3] = {energy->energyYield, energy->sourceQuantiles, energy->retentionLaw};
  const uint32_t counts[3] = {energy->energyYieldCount, energy->sourceQuantilesCount, energy->retentionCount};
  static const char *const names[3] = {"energyYield", "sourceQuantiles", "retentionLaw"};
  static const char *const ranges[3] = {"finite and >= 0", "finite and >= 0", "in [0, 1]"};
  for (int w = 0; w < 3; ++w) {
    if (!tables[w])
      continue;
    if (!gather_law_count_ok(counts[w]))
      return fail(c, VR_E_INVALID, (name + ": " + names[w] + " must have 2 .. 256 entries").c_str());
    for (uint32_t k = 0; k < counts[w]; ++k)
      if (!gather_energy_entry_ok(w, tables[w][k]))
        return fail(c, VR_E_INVALID,
                    (name + ": " + names[w] + "[" + std::to_string(k) + "] is not " + ranges[w] + " (the lowest such index)").c_str());
    set.count[w] = counts[w];
    std::memcpy(set.table + (size_t)w * GATHER_LAW_MAX, tables[w], (size_t)counts[w] * 4);
  }
  if (!(energy->energyMax > 0.f) || !(energy->energyMax <= 3.40282347e+38f))
    return fail(c, VR_E_INVALID, (name + ": energyMax must be finite and > 0").c_str());
  if (!energy->sourceQuantiles && (!(energy->sourceEnergy >= 0.f) || !(energy->sourceEnergy <= 3.40282347e+38f)))
    return fail(c, VR_E_INVALID, (name + ": sourceEnergy must be finite and >= 0").c_str());
  if (energy->energyCut > 1u)
    return fail(c, VR_E_INVALID, (name + ": energyCut is 0 or 1").c_str());
  // (the int64 sum of a primitive holds samples x the largest weight: gather_wmax)
  const double wbound = wboundAngular * (double)gather_law_max(energy->energyYield, energy->energyYieldCount);
  if (!(wbound <= (double)gather_wmax(samples)))
    return fail(c, VR_E_INVALID,
                (name + ": samples x wbound must stay below 2^22, wbound = (g_L max L or g) max Y max Y_E (the int64 sums' range)").c_str());
  set.any = true;
  set.energyMax = energy->energyMax;
  set.sourceEnergy = energy->sourceQuantiles ? 0.f : energy->sourceEnergy;
  const uint32_t Z0 = gather_energy_zeros(energy->energyYield, energy->energyYieldCount);
  set.zeros = energy->energyCut && Z0 >= 2u ? Z0 : 0u;
  return VR_OK;
}

int gather_energy_args(vr_context *c, bool &waited, const GatherEnergySet &set, GatherEnergyArgs &ea) {
  ea = GatherEnergyArgs{};
  if (!set.any)
    return VR_OK;
  VR_TRY(map_grow(c, c->dGatherEnergy, 3 * GATHER_LAW_MAX, waited));
  VR_HIP(c, launch_gather_energy_tables(set.table, c->dGatherEnergy.p, c->stream));
  ea.tables = c->dGatherEnergy.p;
  for (int w = 0; w < 3; ++w)
    ea.count[w] = set.count[w];
  ea.energyMax = set.energyMax;
  ea.sourceEnergy = set.sourceEnergy;
  ea.zeros = set.zeros;
  return VR_OK;
}

int gather_launch(vr_context *c, const TraceParams &p, const GatherArgs &a, const GatherEnergyArgs *ea, unsigned slabs) {
  if (!ea) {
    VR_HIP(c, launch_gather_samples(p, c->geo.geo, c->geo.D, a, slabs, c->stream));
    return VR_OK;
  }
  GatherEnergyArgs e2 = *ea;
  e2.a = a;
  VR_HIP(c, launch_gather_energy(p, c->geo.geo, c->geo.D, e2, slabs, c->stream));
  return VR_OK;
}

// what an energy entry point asks of its spec: the angular call's; a caller's NULL laws means "no law"
static const vr_gather_laws NO_LAWS = {nullptr, 0u, nullptr, 0u, nullptr, 0u};
static int energy_spec(vr_context *c, const char *api, const vr_gather_spec *s, const vr_gather_laws *&laws) {
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

int vr_gather_energy_device(vr_context *c, const vr_gather_spec *s, const vr_gather_laws *laws, const struct vr_gather_energy *energy,
                            uint32_t primFirst, uint32_t primCount, uint32_t samples, float *out, void *stream) {
  if (!c)
    return VR_E_INVALID;
  const char *api = "vr_gather_energy_device";
  VR_TRY(energy_spec(c, api, s, laws));
  return paths_call_device(c, api, laws, primFirst, primCount, samples, s->cosinePower, s->reflection, s->maxBounces, s->reflectivity,
                           s->reflectivityScalar, out, stream, energy);
}

int vr_gather_energy(vr_context *c, const vr_gather_spec *s, const vr_gather_laws *laws, const struct vr_gather_energy *energy,
                     uint32_t primFirst, uint32_t primCount, uint32_t samples, float *out) {
  if (!c)
    return VR_E_INVALID;
  const char *api = "vr_gather_energy";
  VR_TRY(energy_spec(c, api, s, laws));
  return paths_call_host(c, api, laws, primFirst, primCount, samples, s->cosinePower, s->reflection, s->maxBounces, s->reflectivity,
                         s->reflectivityScalar, out, energy);
}

int vr_gather_energy_sums_device(vr_context *c, const vr_gather_spec *s, const vr_gather_laws *laws, const struct vr_gather_energy *energy,
                                 uint32_t primFirst, uint32_t primCount, uint32_t chunkFirst, uint32_t chunks, uint32_t budget,
                                 int64_t *sum, int64_t *sumSq, void *stream) {
  if (!c)
    return VR_E_INVALID;
  const char *api = "vr_gather_energy_sums_device";
  VR_TRY(energy_spec(c, api, s, laws));
  return sums_call_device(c, api, s, laws, primFirst, primCount, chunkFirst, chunks, budget, sum, sumSq, stream, energy);
}

int vr_gather_energy_sums(vr_context *c, const vr_gather_spec *s, const vr_gather_laws *laws, const struct vr_gather_energy *energy,
                          uint32_t primFirst, uint32_t primCount, uint32_t chunkFirst, uint32_t chunks, uint32_t budget, int64_t *sum,
                          int64_t *sumSq) {
  if (!c)
    return VR_E_INVALID;
  const char *api = "vr_gather_energy_sums";
  VR_TRY(energy_spec(c, api, s, laws));
  return sums_call_host(c, api, s, laws, primFirst, primCount, chunkFirst, chunks, budget, sum, sumSq, energy);
}

int vr_gather_energy_adaptive_device(vr_context *c, const vr_gather_spec *s, const vr_gather_laws *laws, const struct vr_gather_energy *energy,
                                     uint32_t primFirst, uint32_t primCount, uint32_t minSamples, uint32_t maxSamples,
                                     float relTarget, float absTarget, float *flux, float *stdErr, uint32_t *samplesUsed,
                                     vr_gather_adaptive_info *info, void *stream) {
  if (!c)
    return VR_E_INVALID;
  const char *api = "vr_gather_energy_adaptive_device";
  VR_TRY(energy_spec(c, api, s, laws));
  return adaptive_call_device(c, api, s, laws, primFirst, primCount, minSamples, maxSamples, relTarget, absTarget, flux, stdErr,
                              samplesUsed, info, stream, energy);
}

int vr_gather_energy_adaptive(vr_context *c, const vr_gather_spec *s, const vr_gather_laws *laws, const struct vr_gather_energy *energy,
                              uint32_t primFirst, uint32_t primCount, uint32_t minSamples, uint32_t maxSamples, float relTarget,
                              float absTarget, float *flux, float *stdErr, uint32_t *samplesUsed, vr_gather_adaptive_info *info) {
  if (!c)
    return VR_E_INVALID;
  const char *api = "vr_gather_energy_adaptive";
  VR_TRY(energy_spec(c, api, s, laws));
  return adaptive_call_host(c, api, s, laws, primFirst, primCount, minSamples, maxSamples, relTarget, absTarget, flux, stdErr,
                            samplesUsed, info, energy);
}

int vr_debug_gather_energy_path(vr_context *c, const vr_gather_spec *s, const vr_gather_laws *laws, const struct vr_gather_energy *energy,
                                uint32_t prim, uint32_t sample, uint32_t maxVertices, uint32_t *vertexIds, float *vertexData,
                                uint32_t *numVertices, uint32_t *end, float *finalDirection3, float *throughput, float *weight,
                                float *energyOut4) {
  if (!c)
    return VR_E_INVALID;
  const char *api = "vr_debug_gather_energy_path";
  VR_TRY(energy_spec(c, api, s, laws));
  return paths_call_debug(c, api, laws, prim, sample, s->cosinePower, s->reflection, s->maxBounces, s->reflectivity,
                          s->reflectivityScalar, maxVertices, vertexIds, vertexData, numVertices, end, finalDirection3, throughput,
                          weight, energy, energyOut4);
}

} // extern "C"
