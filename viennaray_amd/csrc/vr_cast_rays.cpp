// vr_cast_rays.cpp — vr_cast_rays / vr_cast_rays_device: closest-hit queries for the caller's rays against what the last
// prepare left resident (include/viennaray_amd.h has the definition; vr_cast.hip the kernel).  The call prepares nothing
// and touches none of prepared / launched / haveResult: it reads the launch parameters prepare_one kept
// (vr_context::castParams) and refuses when they no longer describe the settings in force.
#include <cmath>
#include <string>

#include "vr_cast.hpp"
#include "vr_context.hpp"

static_assert(VR_CAST_MISS == vr::CAST_MISS && VR_CAST_WALL == vr::CAST_WALL, "vr_cast.hpp's codes are the header's");

namespace vr {

// what both forms refuse before they touch anything; `api`: the entry point's name
static int cast_refusal(vr_context *c, const char *api, const void *org, const void *dir, uint32_t m, uint32_t ld, float tnear,
                        float tmax, uint32_t flags, const void *prim, const void *dist) {
  const std::string name = api;
  if (ld != 2 && ld != 3)
    return fail(c, VR_E_INVALID, (name + ": ld is 2 or 3 floats per row").c_str());
  if (ld == 2 && c->geo.D != 2)
    return fail(c, VR_E_INVALID, (name + ": rows of 2 floats need a 2-D scene").c_str());
  if (!(tnear >= 0.f))
    return fail(c, VR_E_INVALID, (name + ": tnear must not be negative or NaN").c_str());
  if (!(tmax >= 0.f))
    return fail(c, VR_E_INVALID, (name + ": tmax must not be negative or NaN").c_str());
  if (flags & ~VR_CAST_FOLLOW_BOUNDARIES)
    return fail(c, VR_E_INVALID, (name + ": unknown flag bits (VR_CAST_FOLLOW_BOUNDARIES is the only flag)").c_str());
  if (m && (!org || !dir || !prim || !dist))
    return fail(c, VR_E_INVALID, (name + ": origins, directions, prim and dist must not be null").c_str());
  return VR_OK;
}

// the cast needs what a prepare leaves behind — the device build's pair nodes and packed records, the wall table and
// boundary codes of its launch frame, the walk stack — for the geometry and configuration in force (the child order and
// the walls follow the source direction and the boundary conditions: configDirty).  Modelled on map_state_refusal
// Shared with vr_gather_flux.cpp (what: "cast against" / "gather from"): a gather walks what a cast walks, and a new
// staleness condition belongs to both
int resident_scene_refusal(vr_context *c, const char *api, const char *what) {
  if (!c->castValid || !c->haveSetup || c->geometryDirty || c->configDirty || c->castBuild != c->bvhBuilds || c->knobs.hostBuild ||
      c->geo.numPrims == 0 || c->walkStackWaves == 0)
    return fail(c, VR_E_STATE, (std::string(api) + ": nothing to " + what + " for the geometry and configuration in force (call "
                                                   "vr_apply or vr_apply_prepare after setting the geometry, the boundary "
                                                   "conditions or the source direction; not with VR_HOST_BUILD)").c_str());
  return VR_OK;
}
static int cast_state_refusal(vr_context *c, const char *api) { return resident_scene_refusal(c, api, "cast against"); }

// the launch parameters of a walk over the resident scene (shared likewise): what the last prepare kept, the walk stack,
// and the casts' own counter block (the walk's overflow word: an apply's counters stay as they are)
int resident_scene_params(vr_context *c, bool &waited, TraceParams &p) {
  if (!c->dCastCounters.p) {
    VR_TRY(map_grow(c, c->dCastCounters, C_BLOCK, waited));
    VR_HIP(c, hipMemsetAsync(c->dCastCounters.p, 0, C_BLOCK * 8, c->stream));
  }
  p = c->castParams;
  p.walkStack = c->dWalkStack.p;
  p.counters = c->dCastCounters.p;
  return VR_OK;
}

// the kernels, on the context's stream: every pointer is device memory, the arguments have been accepted
static int cast_on_device(vr_context *c, const float *org, const float *dir, uint32_t m, uint32_t ld, float tnear, float tmax,
                          uint32_t flags, int32_t *prim, float *dist, float *hit, uint32_t *bh) {
  bool waited = false;
  const uint32_t *perm = nullptr;
  // The ray sort uses the map's pairs and tables (vr_map_to_points*): both run on c->stream, so one has finished with
  // them before the other starts.  (Beyond 2^31 rays the pairs alone would take 48 GiB: walked in the caller's order.)
  if (m >= read_knobs().castSortMin && m <= (1u << 31)) {
    const size_t tiles = ((size_t)m + 1023) / 1024;
    VR_TRY(map_grow(c, c->dMapKeysA, m, waited));
    VR_TRY(map_grow(c, c->dMapKeysB, m, waited));
    VR_TRY(map_grow(c, c->dMapValsA, m, waited));
    VR_TRY(map_grow(c, c->dMapValsB, m, waited));
    VR_TRY(map_grow(c, c->dMapSortTable, 256 * tiles, waited));
    VR_TRY(map_grow(c, c->dMapScanTmp, 2 * ((256 * tiles) / 2048 + 4) + 64, waited));
    VR_HIP(c, launch_map_keys(org, m, ld, c->geo.D, c->sceneLo, c->sceneHi, c->dMapKeysA.p, c->dMapValsA.p, c->stream));
    VR_HIP(c, launch_sort_pairs(c->dMapKeysA.p, c->dMapValsA.p, c->dMapKeysB.p, c->dMapValsB.p, m, c->dMapSortTable.p,
                                c->dMapScanTmp.p, c->stream));
    perm = c->dMapValsA.p;
  }
  TraceParams p;
  VR_TRY(resident_scene_params(c, waited, p));
  CastArgs a{};
  a.org = org;
  a.dir = dir;
  a.perm = perm;
  a.prim = prim;
  a.dist = dist;
  a.hit = hit;
  a.bh = bh;
  a.m = m;
  a.ld = ld;
  a.groups = (uint32_t)(((uint64_t)m + 63) / 64);
  a.tnear = tnear;
  a.tmax = tmax;
  a.flags = flags;
  a.maxBoundaryHits = c->maxBoundaryHits;
  const unsigned slabs = (unsigned)std::min<size_t>(c->walkStackWaves, 0xFFFFFFFFu);
  VR_HIP(c, launch_cast_rays(p, c->geo.geo, c->geo.D, a, slabs, c->stream));
  return VR_OK;
}

} // namespace vr

extern "C" {

int vr_cast_rays_device(vr_context *c, const float *origins, const float *directions, uint32_t m, uint32_t ld, float tnear,
                        float tmax, uint32_t flags, int32_t *prim, float *dist, float *hitPoints, uint32_t *boundaryHits,
                        void *stream) {
  if (!c)
    return VR_E_INVALID;
  VR_TRY(cast_refusal(c, "vr_cast_rays_device", origins, directions, m, ld, tnear, tmax, flags, prim, dist));
  if (m == 0)
    return VR_OK;
  VR_TRY(cast_state_refusal(c, "vr_cast_rays_device"));
  VR_TRY(hand_over(c, {origins, directions, prim, dist, hitPoints, boundaryHits},
                   "vr_cast_rays_device: origins, directions, prim, dist, hitPoints and boundaryHits must be device memory of "
                   "the context's device",
                   stream));
  VR_TRY(cast_on_device(c, origins, directions, m, ld, tnear, tmax, flags, prim, dist, hitPoints, boundaryHits));
  return caller_waits(c, stream);
}

int vr_cast_rays(vr_context *c, const float *origins3, const float *directions3, uint32_t m, float tnear, float tmax,
                 uint32_t flags, int32_t *prim, float *dist, float *hitPoints, uint32_t *boundaryHits) {
  if (!c)
    return VR_E_INVALID;
  VR_TRY(cast_refusal(c, "vr_cast_rays", origins3, directions3, m, 3, tnear, tmax, flags, prim, dist));
  if (m == 0)
    return VR_OK;
  VR_TRY(cast_state_refusal(c, "vr_cast_rays"));
  VR_HIP(c, hipSetDevice(c->device));
  bool waited = false;
  VR_TRY(map_grow(c, c->dCastOrg, (size_t)m * 3, waited));
  VR_TRY(map_grow(c, c->dCastDir, (size_t)m * 3, waited));
  VR_TRY(map_grow(c, c->dCastPrim, m, waited));
  VR_TRY(map_grow(c, c->dCastDist, m, waited));
  if (hitPoints)
    VR_TRY(map_grow(c, c->dCastHit, (size_t)m * 3, waited));
  if (boundaryHits)
    VR_TRY(map_grow(c, c->dCastBh, m, waited));
  VR_HIP(c, hipMemcpyAsync(c->dCastOrg.p, origins3, (size_t)m * 12, hipMemcpyHostToDevice, c->stream));
  VR_HIP(c, hipMemcpyAsync(c->dCastDir.p, directions3, (size_t)m * 12, hipMemcpyHostToDevice, c->stream));
  VR_TRY(cast_on_device(c, c->dCastOrg.p, c->dCastDir.p, m, 3, tnear, tmax, flags, c->dCastPrim.p, c->dCastDist.p,
                        hitPoints ? c->dCastHit.p : nullptr, boundaryHits ? c->dCastBh.p : nullptr));
  VR_HIP(c, hipMemcpyAsync(prim, c->dCastPrim.p, (size_t)m * 4, hipMemcpyDeviceToHost, c->stream));
  VR_HIP(c, hipMemcpyAsync(dist, c->dCastDist.p, (size_t)m * 4, hipMemcpyDeviceToHost, c->stream));
  if (hitPoints)
    VR_HIP(c, hipMemcpyAsync(hitPoints, c->dCastHit.p, (size_t)m * 12, hipMemcpyDeviceToHost, c->stream));
  if (boundaryHits)
    VR_HIP(c, hipMemcpyAsync(boundaryHits, c->dCastBh.p, (size_t)m * 4, hipMemcpyDeviceToHost, c->stream));
  VR_HIP(c, hipStreamSynchronize(c->stream));
  return VR_OK;
}

} // extern "C"
