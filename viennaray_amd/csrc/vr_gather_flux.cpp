// vr_gather_flux.cpp — vr_gather_flux / vr_gather_flux_device / vr_debug_gather_samples: per-primitive direct flux by rays
// cast from the surface against what the last prepare left resident (include/viennaray_amd.h has the definition;
// vr_gather.hip the kernels, vr_gather.hpp the arithmetic).  Like vr_cast_rays.cpp the calls prepare nothing and touch
// none of prepared / launched / haveResult: they read vr_context::castParams and refuse when it no longer describes the
// settings in force.
#include <cmath>
#include <string>

#include "vr_context.hpp"
#include "vr_gather.hpp"

static_assert(VR_GATHER_NORMAL == vr::GATHER_NORMAL && VR_GATHER_SOURCE == vr::GATHER_SOURCE &&
                  VR_FLUX_FRAC_BITS == vr::GATHER_FRAC_BITS,
              "vr_gather.hpp's constants are the header's");

namespace vr {

// what every form refuses before it touches anything; `api`: the entry point's name
int gather_refusal(vr_context *c, const char *api, uint32_t primFirst, uint32_t primCount, uint32_t samples, float cosinePower,
                   uint32_t mode, const void *emission, const void *out) {
  const std::string name = api;
  if (samples == 0)
    return fail(c, VR_E_INVALID, (name + ": samples must not be 0").c_str());
  if ((uint64_t)primFirst + primCount > c->geo.numPrims)
    return fail(c, VR_E_INVALID, (name + ": the primitive range ends beyond vr_num_primitives").c_str());
  if (!std::isfinite(cosinePower) || cosinePower < 1.f)
    return fail(c, VR_E_INVALID, (name + ": cosinePower must be finite and >= 1").c_str());
  if (mode != VR_GATHER_NORMAL && mode != VR_GATHER_SOURCE)
    return fail(c, VR_E_INVALID, (name + ": mode is VR_GATHER_NORMAL or VR_GATHER_SOURCE").c_str());
  if (mode == VR_GATHER_SOURCE && cosinePower < 2.f)
    return fail(c, VR_E_INVALID, (name + ": VR_GATHER_SOURCE needs cosinePower >= 2 (the weight's variance diverges at 1)").c_str());
  if (mode == VR_GATHER_SOURCE && emission)
    return fail(c, VR_E_INVALID, (name + ": VR_GATHER_SOURCE takes no emission table (its samples look at the source alone)").c_str());
  // (the int64 sum of a primitive holds samples x the largest weight: gather_wmax; a NORMAL weight is at most g)
  if (!((double)gather_g(cosinePower, c->geo.D) <= (double)gather_wmax(samples)))
    return fail(c, VR_E_INVALID, (name + ": samples x g(cosinePower) must stay below 2^22 (the int64 sums' range)").c_str());
  if (primCount && !out)
    return fail(c, VR_E_INVALID, (name + ": out must not be null").c_str());
  return VR_OK;
}

// (the gather walks what a cast walks: one refusal for both, vr_cast_rays.cpp)
static int gather_state_refusal(vr_context *c, const char *api) { return resident_scene_refusal(c, api, "gather from"); }

// launch parameters and the arguments every kernel of this file shares
int gather_params(vr_context *c, bool &waited, TraceParams &p, GatherArgs &a, uint32_t primFirst, uint32_t primCount,
                  uint32_t samples, float cosinePower, uint32_t mode) {
  VR_TRY(resident_scene_params(c, waited, p));
  a = GatherArgs{};
  a.leafOfOrig = c->dLeafOfOrig.p;
  a.primFirst = primFirst;
  a.primCount = primCount;
  a.samples = samples;
  a.mode = mode;
  a.seed = c->rngSeed;
  a.groups = (uint32_t)(((uint64_t)primCount + 63) / 64);
  a.chunks = (uint32_t)(((uint64_t)samples + GATHER_CHUNK - 1) / GATHER_CHUNK);
  a.maxBoundaryHits = c->maxBoundaryHits;
  a.cosinePower = cosinePower;
  a.g = gather_g(cosinePower, c->geo.D);
  a.wmax = gather_wmax(samples);
  a.subs = 1;
  return VR_OK;
}

// a chunk is cut into `subs` runs of samples, work items of their own, until there is an item for every wave the
// walk stack allows (a scene of a few ten thousand primitives at K = 64 is a few hundred (group, chunk) pairs)
void gather_cut_chunks(GatherArgs &a, unsigned slabs) {
  while (a.subs < GATHER_MAX_SUBS && (uint64_t)a.groups * a.chunks * a.subs < slabs)
    a.subs *= 2;
}

// the kernels, on the context's stream: every pointer is device memory, the arguments have been accepted
static int gather_on_device(vr_context *c, uint32_t primFirst, uint32_t primCount, uint32_t samples, float cosinePower,
                            uint32_t mode, const float *emission, float *out) {
  bool waited = false;
  VR_TRY(map_grow(c, c->dGatherAcc, primCount, waited));
  TraceParams p;
  GatherArgs a;
  VR_TRY(gather_params(c, waited, p, a, primFirst, primCount, samples, cosinePower, mode));
  if (primCount == c->geo.numPrims)
    a.leafOfOrig = nullptr; // the whole scene: in leaf order
  a.emission = emission;
  a.acc = c->dGatherAcc.p;
  VR_HIP(c, hipMemsetAsync(c->dGatherAcc.p, 0, (size_t)primCount * 8, c->stream));
  const unsigned slabs = (unsigned)std::min<size_t>(c->walkStackWaves, 0xFFFFFFFFu);
  gather_cut_chunks(a, slabs);
  VR_HIP(c, launch_gather_samples(p, c->geo.geo, c->geo.D, a, slabs, c->stream));
  VR_HIP(c, launch_gather_finish(c->dGatherAcc.p, primCount, samples, out, c->stream));
  return VR_OK;
}

} // namespace vr

extern "C" {

int vr_gather_flux_device(vr_context *c, uint32_t primFirst, uint32_t primCount, uint32_t samples, float cosinePower,
                          uint32_t mode, const float *emission, float *out, void *stream) {
  if (!c)
    return VR_E_INVALID;
  VR_TRY(gather_refusal(c, "vr_gather_flux_device", primFirst, primCount, samples, cosinePower, mode, emission, out));
  if (primCount == 0)
    return VR_OK;
  VR_TRY(gather_state_refusal(c, "vr_gather_flux_device"));
  VR_TRY(hand_over(c, {emission, out}, "vr_gather_flux_device: emission and out must be device memory of the context's device", stream));
  VR_TRY(gather_on_device(c, primFirst, primCount, samples, cosinePower, mode, emission, out));
  return caller_waits(c, stream);
}

int vr_gather_flux(vr_context *c, uint32_t primFirst, uint32_t primCount, uint32_t samples, float cosinePower, uint32_t mode,
                   const float *emission, float *out) {
  if (!c)
    return VR_E_INVALID;
  VR_TRY(gather_refusal(c, "vr_gather_flux", primFirst, primCount, samples, cosinePower, mode, emission, out));
  if (primCount == 0)
    return VR_OK;
  VR_TRY(gather_state_refusal(c, "vr_gather_flux"));
  VR_HIP(c, hipSetDevice(c->device));
  bool waited = false;
  const uint32_t n = c->geo.numPrims;
  VR_TRY(map_grow(c, c->dGatherOut, primCount, waited));
  if (emission) {
    VR_TRY(map_grow(c, c->dGatherEmission, n, waited));
    VR_HIP(c, hipMemcpyAsync(c->dGatherEmission.p, emission, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  }
  VR_TRY(gather_on_device(c, primFirst, primCount, samples, cosinePower, mode, emission ? c->dGatherEmission.p : nullptr,
                          c->dGatherOut.p));
  VR_HIP(c, hipMemcpyAsync(out, c->dGatherOut.p, (size_t)primCount * 4, hipMemcpyDeviceToHost, c->stream));
  VR_HIP(c, hipStreamSynchronize(c->stream));
  return VR_OK;
}

int vr_debug_gather_samples(vr_context *c, uint32_t prim, uint32_t first, uint32_t count, uint32_t mode, float cosinePower,
                            float *origin3, float *normal3, float *directions3) {
  if (!c)
    return VR_E_INVALID;
  // (the checks of the gather itself for a range of one primitive; a run of samples has no count to refuse)
  VR_TRY(gather_refusal(c, "vr_debug_gather_samples", prim, 1, 1, cosinePower, mode, nullptr, origin3));
  if (!normal3 || (count && !directions3))
    return fail(c, VR_E_INVALID, "vr_debug_gather_samples: origin3, normal3 and directions3 must not be null");
  if ((uint64_t)first + count > 0xFFFFFFFFull)
    return fail(c, VR_E_INVALID, "vr_debug_gather_samples: first + count must fit 32 bits");
  VR_TRY(gather_state_refusal(c, "vr_debug_gather_samples"));
  VR_HIP(c, hipSetDevice(c->device));
  bool waited = false;
  VR_TRY(map_grow(c, c->dGatherOut, 6 + (size_t)count * 3, waited));
  TraceParams p;
  GatherArgs a;
  VR_TRY(gather_params(c, waited, p, a, prim, 1, 1, cosinePower, mode));
  float *d = c->dGatherOut.p;
  VR_HIP(c, launch_debug_gather_samples(p, c->geo.geo, c->geo.D, a, first, count, d, d + 3, d + 6, c->stream));
  VR_HIP(c, hipMemcpyAsync(origin3, d, 12, hipMemcpyDeviceToHost, c->stream));
  VR_HIP(c, hipMemcpyAsync(normal3, d + 3, 12, hipMemcpyDeviceToHost, c->stream));
  if (count)
    VR_HIP(c, hipMemcpyAsync(directions3, d + 6, (size_t)count * 12, hipMemcpyDeviceToHost, c->stream));
  VR_HIP(c, hipStreamSynchronize(c->stream));
  return VR_OK;
}

} // extern "C"
