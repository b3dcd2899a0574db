// vr_gather_paths.cpp — vr_gather_paths / vr_gather_paths_device / vr_debug_gather_path: multi-bounce flux by paths traced
// back from the surface (include/viennaray_amd.h has the definition; vr_gather.hip the kernels — the gather's own sample
// loop in its PATH instantiation — vr_gather.hpp the arithmetic).  Like vr_gather_flux.cpp the calls prepare nothing and
// touch none of prepared / launched / haveResult; they refuse what a NORMAL gather refuses, and a reflectivity outside
// [0, 1]: a table is checked on the device by the radiosity solve's kernel, which also leaves it in leaf order.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "vr_context.hpp"
#include "vr_gather.hpp"

static_assert(VR_GATHER_REFLECT_SPECULAR == vr::GATHER_REFLECT_SPECULAR && VR_GATHER_REFLECT_DIFFUSE == vr::GATHER_REFLECT_DIFFUSE &&
                  VR_GATHER_MAX_BOUNCES == vr::GATHER_MAX_BOUNCES && VR_GATHER_PATH_VERTEX_FLOATS == vr::GATHER_PATH_ROW - 1u &&
                  VR_GATHER_END_BOUNCES == vr::GATHER_END_BOUNCES && VR_GATHER_END_ABSORBED == vr::GATHER_END_ABSORBED &&
                  VR_GATHER_END_MISS == vr::GATHER_END_MISS && VR_GATHER_END_BACK == vr::GATHER_END_BACK,
              "vr_gather.hpp's constants are the header's");

namespace vr {

// what every form refuses before it touches anything, beyond the gather's own checks
int paths_refusal(vr_context *c, const char *api, uint32_t primFirst, uint32_t primCount, uint32_t samples, float cosinePower,
                  uint32_t reflection, uint32_t maxBounces, const float *reflectivity, float scalar, const void *out) {
  const std::string name = api;
  VR_TRY(gather_refusal(c, api, primFirst, primCount, samples, cosinePower, VR_GATHER_NORMAL, nullptr, out));
  if (reflection != VR_GATHER_REFLECT_SPECULAR && reflection != VR_GATHER_REFLECT_DIFFUSE)
    return fail(c, VR_E_INVALID, (name + ": reflection is VR_GATHER_REFLECT_SPECULAR or VR_GATHER_REFLECT_DIFFUSE").c_str());
  if (maxBounces > VR_GATHER_MAX_BOUNCES)
    return fail(c, VR_E_INVALID, (name + ": maxBounces must not exceed VR_GATHER_MAX_BOUNCES (65535)").c_str());
  if (!reflectivity && !gather_path_rho_ok(scalar))
    return fail(c, VR_E_INVALID, (name + ": the reflectivity must lie in [0, 1]").c_str());
  return VR_OK;
}

// the table (device memory, by original id) into leaf order and its verdict: ONE word back, the lowest refused index
int paths_table(vr_context *c, const char *api, const float *rho) {
  const uint32_t n = c->geo.numPrims;
  bool waited = false;
  VR_TRY(map_grow(c, c->dPathRho, n, waited));
  VR_TRY(map_grow(c, c->dPathWord, 1, waited));
  VR_HIP(c, hipMemsetAsync(c->dPathWord.p, 0xFF, 4, c->stream));
  VR_HIP(c, launch_radiosity_rho(rho, 0.f, c->dLeafOfOrig.p, n, c->dPathRho.p, c->dPathWord.p, c->stream));
  uint32_t first = 0xFFFFFFFFu;
  VR_HIP(c, hipMemcpyAsync(&first, c->dPathWord.p, 4, hipMemcpyDeviceToHost, c->stream));
  VR_TRY(host_waits(c));
  if (first != 0xFFFFFFFFu)
    return fail(c, VR_E_INVALID, (std::string(api) + ": reflectivity[" + std::to_string(first) +
                                  "] is NaN, negative or above 1 (the lowest such index)")
                                     .c_str());
  return VR_OK;
}

static int paths_args(vr_context *c, bool &waited, TraceParams &p, GatherArgs &a, const GatherLawSet &laws, uint32_t primFirst,
                      uint32_t primCount, uint32_t samples, float cosinePower, uint32_t reflection, uint32_t maxBounces, bool table,
                      float scalar) {
  VR_TRY(gather_params(c, waited, p, a, primFirst, primCount, samples, cosinePower, VR_GATHER_NORMAL));
  VR_TRY(gather_laws_args(c, waited, laws, a));
  a.paths = 1u;
  a.reflection = reflection;
  a.maxBounces = maxBounces;
  a.rho = scalar;
  a.rhoLeaf = table ? c->dPathRho.p : nullptr;
  return VR_OK;
}

// the kernels, on the context's stream: every pointer is device memory, the arguments have been accepted, a table
// (table: c->dPathRho holds it) has passed paths_table
static int paths_on_device(vr_context *c, const GatherLawSet &laws, const GatherEnergySet &energy, uint32_t primFirst,
                           uint32_t primCount, uint32_t samples, float cosinePower, uint32_t reflection, uint32_t maxBounces,
                           bool table, float scalar, float *out) {
  bool waited = false;
  VR_TRY(map_grow(c, c->dGatherAcc, primCount, waited));
  TraceParams p;
  GatherArgs a;
  VR_TRY(paths_args(c, waited, p, a, laws, primFirst, primCount, samples, cosinePower, reflection, maxBounces, table, scalar));
  GatherEnergyArgs ea;
  VR_TRY(gather_energy_args(c, waited, energy, ea));
  if (primCount == c->geo.numPrims)
    a.leafOfOrig = nullptr; // the whole scene: in leaf order
  a.acc = c->dGatherAcc.p;
  VR_HIP(c, hipMemsetAsync(c->dGatherAcc.p, 0, (size_t)primCount * 8, c->stream));
  const unsigned slabs = (unsigned)std::min<size_t>(c->walkStackWaves, 0xFFFFFFFFu);
  gather_cut_chunks(a, slabs);
#ifdef VR_DIAG
  VR_HIP(c, hipMemsetAsync(p.counters + C_DIAG, 0, 16, c->stream));
#endif
  VR_TRY(gather_launch(c, p, a, energy.any ? &ea : nullptr, slabs));
  VR_HIP(c, launch_gather_finish(c->dGatherAcc.p, primCount, samples, out, c->stream));
#ifdef VR_DIAG
  { // the segment loop's lane occupancy (tools/gather_paths_bench.py reads the line): a round of segments occupies the
    // wave until its longest path has finished the segment; a lane is useful in it while its own path still walks
    unsigned long long dg[2];
    VR_HIP(c, hipStreamSynchronize(c->stream));
    VR_HIP(c, hipMemcpy(dg, p.counters + C_DIAG, sizeof(dg), hipMemcpyDeviceToHost));
    std::fprintf(stderr, "diag gather paths: rounds %llu segments %llu paths %llu\n", dg[0], dg[1],
                 (unsigned long long)primCount * samples);
  }
#endif
  return VR_OK;
}


int paths_call_device(vr_context *c, const char *api, const vr_gather_laws *lawsIn, uint32_t primFirst, uint32_t primCount,
                      uint32_t samples, float cosinePower, uint32_t reflection, uint32_t maxBounces, const float *reflectivity,
                      float reflectivityScalar, float *out, void *stream, const struct vr_gather_energy *energyIn) {
  VR_TRY(paths_refusal(c, api, primFirst, primCount, samples, cosinePower, reflection, maxBounces, reflectivity, reflectivityScalar, out));
  GatherLawSet laws;
  VR_TRY(gather_laws_refusal(c, api, lawsIn, cosinePower, samples, laws));
  GatherEnergySet energy;
  VR_TRY(gather_energy_refusal(c, api, energyIn, laws.wbound, samples, energy));
  VR_TRY(resident_scene_refusal(c, api, "gather from"));
  VR_TRY(hand_over(c, {reflectivity, out},
                   (std::string(api) + ": reflectivity and out must be device memory of the context's device").c_str(), stream));
  if (reflectivity)
    VR_TRY(paths_table(c, api, reflectivity));
  if (primCount == 0)
    return caller_waits(c, stream);
  VR_TRY(paths_on_device(c, laws, energy, primFirst, primCount, samples, cosinePower, reflection, maxBounces, reflectivity != nullptr,
                         reflectivityScalar, out));
  return caller_waits(c, stream);
}

int paths_call_host(vr_context *c, const char *api, const vr_gather_laws *lawsIn, uint32_t primFirst, uint32_t primCount,
                    uint32_t samples, float cosinePower, uint32_t reflection, uint32_t maxBounces, const float *reflectivity,
                    float reflectivityScalar, float *out, const struct vr_gather_energy *energyIn) {
  VR_TRY(paths_refusal(c, api, primFirst, primCount, samples, cosinePower, reflection, maxBounces, reflectivity, reflectivityScalar, out));
  GatherLawSet laws;
  VR_TRY(gather_laws_refusal(c, api, lawsIn, cosinePower, samples, laws));
  GatherEnergySet energy;
  VR_TRY(gather_energy_refusal(c, api, energyIn, laws.wbound, samples, energy));
  VR_TRY(resident_scene_refusal(c, api, "gather from"));
  VR_HIP(c, hipSetDevice(c->device));
  bool waited = false;
  const uint32_t n = c->geo.numPrims;
  if (reflectivity) {
    VR_TRY(map_grow(c, c->dPathIn, n, waited));
    VR_HIP(c, hipMemcpyAsync(c->dPathIn.p, reflectivity, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    VR_TRY(paths_table(c, api, c->dPathIn.p));
  }
  if (primCount == 0)
    return VR_OK;
  VR_TRY(map_grow(c, c->dGatherOut, primCount, waited));
  VR_TRY(paths_on_device(c, laws, energy, primFirst, primCount, samples, cosinePower, reflection, maxBounces, reflectivity != nullptr,
                         reflectivityScalar, c->dGatherOut.p));
  VR_HIP(c, hipMemcpyAsync(out, c->dGatherOut.p, (size_t)primCount * 4, hipMemcpyDeviceToHost, c->stream));
  VR_HIP(c, hipStreamSynchronize(c->stream));
  return VR_OK;
}

int paths_call_debug(vr_context *c, const char *api, const vr_gather_laws *lawsIn, uint32_t prim, uint32_t sample, float cosinePower,
                     uint32_t reflection, uint32_t maxBounces, const float *reflectivity, float reflectivityScalar,
                     uint32_t maxVertices, uint32_t *vertexIds, float *vertexData, uint32_t *numVertices, uint32_t *end,
                     float *finalDirection3, float *throughput, float *weight, const struct vr_gather_energy *energyIn, float *energyOut4) {
  const std::string name = api;
  // (the checks of the call itself for a range of one primitive and one sample; c: a non-null `out`)
  VR_TRY(paths_refusal(c, api, prim, 1, 1, cosinePower, reflection, maxBounces, reflectivity, reflectivityScalar, c));
  GatherLawSet laws;
  VR_TRY(gather_laws_refusal(c, api, lawsIn, cosinePower, 1, laws));
  GatherEnergySet energy;
  VR_TRY(gather_energy_refusal(c, api, energyIn, laws.wbound, 1, energy));
  if (maxVertices && (!vertexIds || !vertexData))
    return fail(c, VR_E_INVALID, (name + ": vertexIds and vertexData must not be null with maxVertices > 0").c_str());
  if (maxVertices > VR_GATHER_MAX_BOUNCES + 2u)
    return fail(c, VR_E_INVALID, (name + ": maxVertices must not exceed VR_GATHER_MAX_BOUNCES + 2").c_str());
  if (sample >= (1u << 22)) // (samples x g <= 2^22: no call has a sample beyond)
    return fail(c, VR_E_INVALID, (name + ": sample must be below 2^22, the most samples a call can have").c_str());
  VR_TRY(resident_scene_refusal(c, api, "gather from"));
  VR_HIP(c, hipSetDevice(c->device));
  bool waited = false;
  const uint32_t n = c->geo.numPrims;
  if (reflectivity) {
    VR_TRY(map_grow(c, c->dPathIn, n, waited));
    VR_HIP(c, hipMemcpyAsync(c->dPathIn.p, reflectivity, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    VR_TRY(paths_table(c, api, c->dPathIn.p));
  }
  const size_t rows = (size_t)maxVertices * GATHER_PATH_ROW;
  VR_TRY(map_grow(c, c->dGatherOut, rows + GATHER_PATH_TAIL + 4u, waited)); // (4: the energy path's {u, E0, P, e})
  VR_TRY(map_grow(c, c->dGatherAcc, 1, waited));
  TraceParams p;
  GatherArgs a;
  VR_TRY(paths_args(c, waited, p, a, laws, prim, 1, 1, cosinePower, reflection, maxBounces, reflectivity != nullptr,
                    reflectivityScalar));
  GatherEnergyArgs ea;
  VR_TRY(gather_energy_args(c, waited, energy, ea));
  if (c->walkStackWaves == 0)
    return fail(c, VR_E_STATE, (name + ": the walk stack has no slab").c_str());
  a.acc = c->dGatherAcc.p; // (the kernel is the gather's: the one sample's sum goes where a gather's would)
  VR_HIP(c, hipMemsetAsync(c->dGatherAcc.p, 0, 8, c->stream));
  float *d = c->dGatherOut.p;
  if (energy.any) {
    ea.a = a;
    VR_HIP(c, launch_debug_gather_energy_path(p, c->geo.geo, c->geo.D, ea, sample, maxVertices, d, d + rows, d + rows + GATHER_PATH_TAIL,
                                              c->stream));
  } else {
    VR_HIP(c, launch_debug_gather_path(p, c->geo.geo, c->geo.D, a, sample, maxVertices, d, d + rows, c->stream));
  }
  std::vector<float> host(rows + GATHER_PATH_TAIL + 4u);
  VR_HIP(c, hipMemcpyAsync(host.data(), d, host.size() * 4, hipMemcpyDeviceToHost, c->stream));
  VR_HIP(c, hipStreamSynchronize(c->stream));
  auto word = [](float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
  };
  const float *tail = host.data() + rows;
  const uint32_t count = word(tail[0]);
  for (uint32_t v = 0; v < std::min(count, maxVertices); ++v) {
    const float *row = host.data() + (size_t)v * GATHER_PATH_ROW;
    vertexIds[v] = word(row[0]);
    std::memcpy(vertexData + (size_t)v * VR_GATHER_PATH_VERTEX_FLOATS, row + 1, VR_GATHER_PATH_VERTEX_FLOATS * 4);
  }
  if (numVertices)
    *numVertices = count;
  if (end)
    *end = word(tail[1]);
  if (finalDirection3)
    std::memcpy(finalDirection3, tail + 2, 12);
  if (throughput)
    *throughput = tail[5];
  if (weight)
    *weight = tail[6];
  if (energy.any && energyOut4)
    std::memcpy(energyOut4, tail + GATHER_PATH_TAIL, 16);
  return VR_OK;
}

} // namespace vr

using namespace vr;

extern "C" {

int vr_gather_paths_device(vr_context *c, uint32_t primFirst, uint32_t primCount, uint32_t samples, float cosinePower,
                           uint32_t reflection, uint32_t maxBounces, const float *reflectivity, float reflectivityScalar, float *out,
                           void *stream) {
  if (!c)
    return VR_E_INVALID;
  return paths_call_device(c, "vr_gather_paths_device", nullptr, primFirst, primCount, samples, cosinePower, reflection, maxBounces,
                           reflectivity, reflectivityScalar, out, stream);
}

int vr_gather_paths(vr_context *c, uint32_t primFirst, uint32_t primCount, uint32_t samples, float cosinePower, uint32_t reflection,
                    uint32_t maxBounces, const float *reflectivity, float reflectivityScalar, float *out) {
  if (!c)
    return VR_E_INVALID;
  return paths_call_host(c, "vr_gather_paths", nullptr, primFirst, primCount, samples, cosinePower, reflection, maxBounces,
                         reflectivity, reflectivityScalar, out);
}

int vr_debug_gather_path(vr_context *c, uint32_t prim, uint32_t sample, float cosinePower, uint32_t reflection, uint32_t maxBounces,
                         const float *reflectivity, float reflectivityScalar, uint32_t maxVertices, uint32_t *vertexIds,
                         float *vertexData, uint32_t *numVertices, uint32_t *end, float *finalDirection3, float *throughput,
                         float *weight) {
  if (!c)
    return VR_E_INVALID;
  return paths_call_debug(c, "vr_debug_gather_path", nullptr, prim, sample, cosinePower, reflection, maxBounces, reflectivity,
                          reflectivityScalar, maxVertices, vertexIds, vertexData, numVertices, end, finalDirection3, throughput,
                          weight);
}

} // extern "C"
