// vr_api.cpp — the C ABI (include/viennaray_amd.h) on top of the host setup (vr_host.cpp) and the HIP kernels
// (the .hip files: vr_trace.hip has their map).  This file: create / destroy and the setters.  The rest of the ABI, by stage:
//   vr_context.hpp  struct vr_context and what the files below share
//   vr_source.hpp   RaySource: the ray source in force, its one transition, the questions the stages ask about it
//   vr_source.cpp   the setters of the ray sources (grid, host rays, surface source, source model)
//   vr_knobs.cpp    read_knobs: the tuning switches of the environment
//   vr_models.cpp   run-time particle and source models (vr_register_particle_model, vr_register_source_model)
//   vr_scene.cpp    host mirrors of the resident geometry, build_scene
//   vr_prepare.cpp  vr_apply_prepare and its stages
//   vr_apply.cpp    vr_apply_launch / _finish, vr_apply, vr_apply_sharded
//   vr_results.cpp  flux, TraceInfo and data-log getters, normalise, smooth, areas, values at the caller's points
//   vr_cast_rays.cpp  closest-hit queries for the caller's rays (vr_cast_rays*)
//   vr_debug.cpp    the vr_debug_* entry points
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "vr_context.hpp"
#include "vr_particles.hpp"

namespace vr {

int fail(vr_context *c, int code, const char *msg) {
  if (c)
    c->err = msg;
  return code;
}

// ---- the hand-over of the device entry points -------------------------------
// An entry point that takes (or, vr_get_flux_device, fills) a buffer in device memory works on the context's own stream,
// between hand_over and one of two ends.  hand_over selects the device, refuses a buffer that is not device memory of the
// context's device — before that nothing of the context is touched — and makes c->stream wait for what the caller's
// stream (nullptr: the null stream) holds now.  The ends:
//   host_waits     the host waits for c->stream: where a verdict or bounds must come back.  On return the library is done
//                  with the caller's buffers, and an apply launched earlier has finished.
//   caller_waits   the caller's stream waits for what c->stream holds now: where nothing comes back.  Nothing waits on the
//                  host.  The caller may reuse its buffers in the order of its stream; to overwrite them from the host or
//                  free them it synchronises its stream first.
// Every kernel of an apply runs on c->stream, so what an entry point writes there is behind an apply launched earlier,
// and what such an apply may still be reading is only ever replaced in that order.  A resident buffer that has to MOVE
// (DevBuf::ensure frees the old one) is moved after host_waits only; at steady state, inputs that do not grow, none does.
// Per entry point:
//   vr_set_disks_device           host_waits, once (the box comes back).  Buffers: free on return.  The resident disk
//                                 arrays are rewritten behind an earlier apply, which has finished on return.
//   vr_set_triangles_device       host_waits once, for the scan's verdict and box, then caller_waits for the copy.
//                                 Buffers: in stream order.  An earlier apply has finished before anything resident is
//                                 touched.
//   vr_set_material_ids_device    caller_waits.  Buffers: in stream order.  The ids are rewritten behind an earlier apply.
//   vr_set_global_data_device     caller_waits.  Buffers: in stream order.  The row is rewritten behind an earlier apply;
//                                 the other rows stay as they are (lay_global_rows re-lays them when they have to move).
//   vr_set_surface_source_device  host_waits, once (the verdict comes back).  Buffers: free on return.  An earlier apply
//                                 reads the previous tables, which are swapped out only once it has finished.
//   vr_get_flux_device            caller_waits (vr_results.cpp; with smoothing one word comes back in between).  The
//                                 result is ready in stream order.
//   vr_map_to_points_device,      caller_waits (vr_results.cpp).  The result is ready in stream order; the map's work buffers
//   vr_get_flux_at_points_device  grow behind host_waits (the first call, a larger m), otherwise nothing waits on the host.
//   vr_cast_rays_device           caller_waits (vr_cast_rays.cpp).  The results are ready in stream order; the ray sort's
//                                 buffers (the map's) grow behind host_waits, otherwise nothing waits on the host.

// `p` is device memory of `device` (hipMalloc / a torch tensor's storage; not host, pinned or managed memory)
static bool is_device_memory_of(const void *p, int device) {
  hipPointerAttribute_t a{};
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError(); // (an unregistered host pointer is an error of this call on some runtimes: not a sticky one)
    return false;
  }
  return a.type == hipMemoryTypeDevice && a.device == device;
}
// (`refusal`: the entry point's own wording; a buffer of no elements is passed as nullptr and not looked at)
int hand_over(vr_context *c, std::initializer_list<const void *> buffers, const char *refusal, void *stream) {
  VR_HIP(c, hipSetDevice(c->device));
  for (const void *p : buffers)
    if (p && !is_device_memory_of(p, c->device))
      return fail(c, VR_E_INVALID, refusal);
  if (!c->evIn)
    VR_HIP(c, hipEventCreateWithFlags(&c->evIn, hipEventDisableTiming));
  VR_HIP(c, hipEventRecord(c->evIn, (hipStream_t)stream));
  VR_HIP(c, hipStreamWaitEvent(c->stream, c->evIn, 0));
  return VR_OK;
}
int host_waits(vr_context *c) {
  VR_HIP(c, hipStreamSynchronize(c->stream));
  return VR_OK;
}
int caller_waits(vr_context *c, void *stream) {
  if (!c->evOut)
    VR_HIP(c, hipEventCreateWithFlags(&c->evOut, hipEventDisableTiming));
  VR_HIP(c, hipEventRecord(c->evOut, c->stream));
  VR_HIP(c, hipStreamWaitEvent((hipStream_t)stream, c->evOut, 0));
  return VR_OK;
}

// ---- the geometry commit ------------------------------------------------------
// nothing derived from the previous geometry holds
// (hostNeighborsValid also for triangles, whose neighbourhood host_set_triangles has just written as ensure_host_neighbors
//  would: empty lists for every triangle, whatever the flag says.)
static void invalidate_geometry(vr_context *c) {
  c->hostNeighborsValid = false;
  c->areasValid = false;
  c->boundFlux = nullptr;
  c->geometryDirty = true;
  c->configDirty = true;
  c->prepared = c->haveResult = false;
}

// the material ids of a geometry with the same primitive count are kept, and reset to 0 otherwise: here for ids that
// were set from the device (commit_geometry makes the host's n zeros)
static void material_ids_follow(vr_context *c, uint32_t n) {
  if (c->materialOnDevice) {
    if (c->materialCount == n)
      return;
    c->materialOnDevice = false;
    c->materialIds.clear();
    c->materialStale = true;
  } else if (c->materialIds.size() != n) {
    c->materialStale = true;
  }
}

// Every geometry setter ends here, with nothing left that can fail: `d` describes what the mirror (a host setter) or the
// resident buffers (fromDevice) hold now.  A device setter whose work failed after it had begun to write commits
// GeometryDesc{}: "no geometry", not half of one.  The order: material_ids_follow first, it compares the new count with
// the ids as the previous geometry left them, which the zero-fill below replaces; the rest is independent of each other.
static void commit_geometry(vr_context *c, const GeometryDesc &d, bool fromDevice) {
  material_ids_follow(c, d.numPrims);
  invalidate_geometry(c);
  if (fromDevice)
    c->geo.clear(); // (the previous geometry's: ensure_host_geometry fills it when a host path asks)
  static_cast<GeometryDesc &>(c->geo) = d;
  if (!c->materialOnDevice && c->materialIds.size() != d.numPrims)
    c->materialIds.assign(d.numPrims, 0);
  c->geoOnDevice = fromDevice;
  c->hostGeoValid = false;
}

// a message that a host setter and its device twin share (on purpose under the host setter's name: the device twin
// applies the host loop's checks and reports what it would; the surface source's: vr_source.cpp)
static const char kTriangleIndexError[] = "vr_set_triangles: vertex index out of range"; // (the device: + the triangle)

// vector vecIdx and every one behind it are gone (vr_set_global_data* with no data)
static void drop_global_from(vr_context *c, uint32_t vecIdx) {
  c->globalRows.resize(c->globalVecs.size());
  if (vecIdx < c->globalVecs.size()) {
    c->globalVecs.resize(vecIdx);
    c->globalRows.resize(vecIdx);
  }
  c->globalRowsLaid = std::min(c->globalRowsLaid, (uint32_t)c->globalVecs.size());
}

} // namespace vr

extern "C" {

const char *vr_version(void) { return "viennaray_amd 0.1 (gfx950)"; }

int vr_device_available(void) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  return (e == hipSuccess && n > 0) ? 1 : 0;
}

int vr_create(vr_context **out, int device) {
  if (!out)
    return VR_E_INVALID;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n)
    return VR_E_HIP;
  vr_context *c = new vr_context();
  c->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess) {
    delete c;
    return VR_E_HIP;
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess)
    c->numCUs = prop.multiProcessorCount;
  *out = c;
  return VR_OK;
}

void vr_destroy(vr_context *c) {
  if (!c)
    return;
  (void)hipSetDevice(c->device);
  if (c->stream)
    (void)hipStreamSynchronize(c->stream);
  for (auto &sm : c->sourceModels)
    if (sm.module)
      (void)hipModuleUnload(sm.module);
  for (auto &um : c->userModels) {
    if (um.module)
      (void)hipModuleUnload(um.module);
    if (um.statsModule)
      (void)hipModuleUnload(um.statsModule);
  }
  c->evK.insert(c->evK.end(), c->evG.begin(), c->evG.end());
  c->evK.insert(c->evK.end(), {c->evIn, c->evOut, c->ev0, c->ev1});
  for (hipEvent_t e : c->evK)
    if (e)
      (void)hipEventDestroy(e);
  if (c->stream)
    (void)hipStreamDestroy(c->stream);
  delete c; // (every DevBuf frees its memory: the device is selected and idle)
}

const char *vr_last_error(const vr_context *c) { return c ? c->err.c_str() : "null context"; }

// ---- geometry ---------------------------------------------------------------
int vr_set_disks(vr_context *c, const float *points, const float *normals, uint32_t n, float gridDelta,
                 float diskRadius, int D) {
  if (!c || !points || !normals || (D != 2 && D != 3) || n >= (1u << 27))
    return fail(c, VR_E_INVALID, "vr_set_disks: bad argument");
  commit_geometry(c, host_set_disks(c->geo, points, normals, n, gridDelta, diskRadius, D), false);
  return VR_OK;
}

// vr_set_disks for rows that live on the device: one kernel packs them into the builder's buffers and reduces the
// bounding box; six floats come back.
int vr_set_disks_device(vr_context *c, const float *points, const float *normals, uint32_t n, uint32_t ld,
                        float gridDelta, float diskRadius, int D, void *stream) {
  if (!c || !points || !normals || (D != 2 && D != 3) || n >= (1u << 27))
    return fail(c, VR_E_INVALID, "vr_set_disks_device: bad argument");
  if (ld != 2 && ld != 3)
    return fail(c, VR_E_INVALID, "vr_set_disks_device: ld (floats per row) must be 2 or 3");
  if (ld == 2 && D != 2)
    return fail(c, VR_E_INVALID, "vr_set_disks_device: rows of 2 floats need D == 2");
  VR_TRY(hand_over(c, {n ? points : nullptr, n ? normals : nullptr},
                   "vr_set_disks_device: points / normals are not device memory of the context's device", stream));
  GeometryDesc d{D, 0, n, 0, gridDelta, host_disk_radius(gridDelta, diskRadius, D)}; // (its box: below)
  const int r = [&]() -> int { // from here on the resident buffers no longer hold the previous geometry
    // (the kernel takes both passes in one, so the buffers are needed before the call's one synchronisation: where one
    //  of them has to move, an apply launched earlier must have finished first)
    if (!c->dPoints3.holds((size_t)n * 3) || !c->dNormal3.holds((size_t)n * 3) || !c->dDisk4.holds((size_t)n * 4))
      VR_TRY(host_waits(c));
    VR_HIP(c, c->dPoints3.ensure((size_t)n * 3));
    VR_HIP(c, c->dNormal3.ensure((size_t)n * 3));
    VR_HIP(c, c->dDisk4.ensure((size_t)n * 4));
    VR_HIP(c, c->dIngestKeys.ensure(ingest_partials_entries()));
    VR_HIP(c, c->dIngestBounds.ensure(6));
    VR_HIP(c, launch_ingest_disks(points, normals, n, ld, D, d.diskRadius, c->dPoints3.p, c->dNormal3.p, c->dDisk4.p,
                                  c->dIngestKeys.p, c->dIngestBounds.p, c->stream));
    float b[6];
    VR_HIP(c, hipMemcpyAsync(b, c->dIngestBounds.p, sizeof(b), hipMemcpyDeviceToHost, c->stream));
    VR_TRY(host_waits(c));
    for (int k = 0; k < D; ++k) {
      d.minC[k] = b[k];
      d.maxC[k] = b[3 + k];
    }
    return VR_OK;
  }();
  commit_geometry(c, r == VR_OK ? d : GeometryDesc{}, true);
  return r;
}

int vr_set_triangles(vr_context *c, const float *verts, uint32_t nverts, const uint32_t *tris, uint32_t ntris,
                     float gridDelta, int D) {
  if (!c || !verts || !tris || (D != 2 && D != 3) || ntris >= (1u << 27))
    return fail(c, VR_E_INVALID, "vr_set_triangles: bad argument");
  for (size_t i = 0; i < (size_t)ntris * 3; ++i)
    if (tris[i] >= nverts)
      return fail(c, VR_E_INVALID, kTriangleIndexError);
  commit_geometry(c, host_set_triangles(c->geo, verts, nverts, tris, ntris, gridDelta, D), false);
  return VR_OK;
}

// vr_set_triangles for a mesh that lives on the device, in two passes (vr_ingest.hip).  The first reads the caller's
// buffers only — box of all vertices, lowest triangle with an index out of range — and its seven words are the call's one
// synchronisation with the host; nothing resident is touched before they say that the mesh is good.  The second copies
// both buffers and makes the normals and areas of host_set_triangles.
int vr_set_triangles_device(vr_context *c, const float *verts, uint32_t nverts, const uint32_t *tris, uint32_t ntris,
                            float gridDelta, int D, void *stream) {
  // (nverts < 2^31: the box reduction's keys carry the row in 31 bits)
  if (!c || (nverts && !verts) || (ntris && !tris) || (D != 2 && D != 3) || ntris >= (1u << 27) || nverts >= (1u << 31))
    return fail(c, VR_E_INVALID, "vr_set_triangles_device: bad argument");
  VR_TRY(hand_over(c, {nverts ? verts : nullptr, ntris ? tris : nullptr},
                   "vr_set_triangles_device: verts / tris are not device memory of the context's device", stream));
  VR_HIP(c, c->dIngestKeys.ensure(ingest_partials_entries()));
  VR_HIP(c, c->dIngestBounds.ensure(7));
  VR_HIP(c, launch_scan_mesh(verts, nverts, tris, ntris, c->dIngestKeys.p, c->dIngestBounds.p,
                             reinterpret_cast<unsigned *>(c->dIngestBounds.p + 6), c->stream));
  float b[7];
  VR_HIP(c, hipMemcpyAsync(b, c->dIngestBounds.p, sizeof(b), hipMemcpyDeviceToHost, c->stream));
  VR_TRY(host_waits(c));
  uint32_t bad;
  std::memcpy(&bad, &b[6], 4);
  if (bad != 0xFFFFFFFFu)
    return fail(c, VR_E_INVALID, (kTriangleIndexError + (" (triangle " + std::to_string(bad) + ")")).c_str());
  GeometryDesc d{D, 1, ntris, nverts, gridDelta, 0.f};
  for (int k = 0; k < 3 && nverts; ++k) { // (no vertices: the zeros of host_set_triangles)
    d.minC[k] = b[k];
    d.maxC[k] = b[3 + k];
  }
  const int r = [&]() -> int { // from here on the resident buffers no longer hold the previous geometry
    VR_HIP(c, c->dVerts.ensure((size_t)nverts * 3));
    VR_HIP(c, c->dTris.ensure((size_t)ntris * 3));
    VR_HIP(c, c->dNormal3.ensure((size_t)ntris * 3));
    VR_HIP(c, c->dTriAreas.ensure(ntris));
    VR_HIP(c, launch_pack_mesh(verts, nverts, tris, ntris, D, c->dVerts.p, c->dTris.p, c->dNormal3.p, c->dTriAreas.p,
                               c->stream));
    return caller_waits(c, stream);
  }();
  commit_geometry(c, r == VR_OK ? d : GeometryDesc{}, true);
  return r;
}

int vr_set_material_ids(vr_context *c, const int32_t *ids, uint32_t n) {
  if (!c || !ids)
    return fail(c, VR_E_INVALID, "vr_set_material_ids: bad argument");
  c->materialIds.assign(ids, ids + n);
  c->materialOnDevice = false;
  c->materialStale = true;
  c->prepared = false;
  c->configDirty = true;
  return VR_OK;
}

// vr_set_material_ids for ids that live on the device: one device-to-device copy; materialIds is not filled.  Only the
// sticking maps follow from the ids: nothing else is redone.
int vr_set_material_ids_device(vr_context *c, const int32_t *ids, uint32_t n, void *stream) {
  if (!c || (n && !ids))
    return fail(c, VR_E_INVALID, "vr_set_material_ids_device: bad argument");
  if (n == 0) { // (as vr_set_material_ids with no ids: every primitive has id 0)
    c->materialIds.clear();
    c->materialOnDevice = false;
    c->materialStale = true;
  } else {
    VR_TRY(hand_over(c, {ids}, "vr_set_material_ids_device: ids are not device memory of the context's device", stream));
    if (!c->dMaterialIds.holds(n)) {
      VR_TRY(host_waits(c)); // (the buffer moves: nothing may still read it)
      VR_HIP(c, c->dMaterialIds.ensure(n));
    }
    VR_HIP(c, hipMemcpyAsync(c->dMaterialIds.p, ids, (size_t)n * 4, hipMemcpyDeviceToDevice, c->stream));
    VR_TRY(caller_waits(c, stream));
    c->materialCount = n;
    c->materialOnDevice = true;
    c->materialStale = false;
  }
  c->particleDirty = true;
  c->prepared = false;
  return VR_OK;
}

// ---- configuration ----------------------------------------------------------
int vr_set_boundary_conditions(vr_context *c, const int32_t *bcs, int n) {
  if (!c || !bcs || n < 1 || n > 3)
    return fail(c, VR_E_INVALID, "vr_set_boundary_conditions: bad argument");
  for (int i = 0; i < n; ++i) {
    if (bcs[i] < 0 || bcs[i] > 2)
      return fail(c, VR_E_INVALID, "vr_set_boundary_conditions: unknown condition");
    c->bcs[i] = bcs[i];
  }
  c->prepared = false;
  c->configDirty = true;
  return VR_OK;
}
int vr_set_source_direction(vr_context *c, int d) {
  if (!c || d < 0 || d > 5)
    return fail(c, VR_E_INVALID, "vr_set_source_direction: bad argument");
  c->sourceDirection = d;
  c->prepared = false;
  c->configDirty = true;
  return VR_OK;
}
int vr_set_primary_direction(vr_context *c, const float *d) {
  if (!c)
    return VR_E_INVALID;
  if (d) {
    std::memcpy(c->primaryDirection, d, 12);
    c->usePrimaryDirection = true;
  } else {
    c->usePrimaryDirection = false;
  }
  c->prepared = false;
  c->configDirty = true;
  return VR_OK;
}
static bool spec_from_pod(const vr_context *c, const vr_particle *p, ParticleSpec &sp) {
  if (!p || p->kind < 0)
    return false;
  const bool user = p->kind >= VR_PARTICLE_USER_BASE;
  if (user ? (size_t)(p->kind - VR_PARTICLE_USER_BASE) >= c->userModels.size() : p->kind >= Particles::count)
    return false;
  sp = ParticleSpec{};
  sp.kind = p->kind;
  sp.userModel = user ? p->kind - VR_PARTICLE_USER_BASE : -1;
  sp.kernelKind = user ? VR_BUILTIN_MODELS : p->kind;
  sp.numData = user ? (uint32_t)c->userModels[sp.userModel].numData : (uint32_t)Particles::numData(p->kind);
  sp.sticking = p->sticking;
  // rayParticle.hpp:158,199: only SpecularParticle-like particles carry a source power of their own
  sp.sourcePower = (p->kind == VR_PARTICLE_DIFFUSE || p->kind == VR_PARTICLE_DIFFUSE_COSINE ||
                    p->kind == VR_PARTICLE_COVERAGE_STICKING)
                       ? 1.f
                       : p->sourcePower;
  sp.coneAngle = p->coneAngle;
  sp.meanFreePath = p->meanFreePath;
  std::memcpy(sp.params, p->params, sizeof(sp.params));
  if (p->kind == VR_PARTICLE_CONED_COSINE)
    sp.params[0] = p->coneAngle; // (the model reads its cone angle from params[0])
  if (p->numMaterialSticking > 0 && p->materialIds && p->materialSticking) {
    sp.matIds.assign(p->materialIds, p->materialIds + p->numMaterialSticking);
    sp.matVals.assign(p->materialSticking, p->materialSticking + p->numMaterialSticking);
  }
  return true;
}

int vr_set_particles(vr_context *c, const vr_particle *list, uint32_t n) {
  if (!c || !list || n == 0 || n > 64)
    return fail(c, VR_E_INVALID, "vr_set_particles: between 1 and 64 particles");
  std::vector<ParticleSpec> specs(n);
  uint32_t total = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (!spec_from_pod(c, &list[i], specs[i]))
      return fail(c, VR_E_INVALID, "vr_set_particle: unknown particle kind (not in the device registry, not registered)");
    total += specs[i].numData;
  }
  c->specs = std::move(specs);
  c->particleDirty = true;
  c->totalData = total;
  // a caller's accumulator buffer (vr_bind_flux_accumulators) stays bound while it still has the right size: numPrims x
  // data labels of ALL particles; it is dropped only when the number of planes changed
  if (c->boundFlux && c->boundFluxN != c->geo.numPrims * c->totalPlanes()) {
    c->boundFlux = nullptr;
    c->boundFluxN = 0;
  }
  c->prepared = false;
  return VR_OK;
}

int vr_set_particle(vr_context *c, const vr_particle *p) { return vr_set_particles(c, p, 1); }

// Trace::setGlobalData (rayTrace.hpp:137-145): vector `vecIdx` of the borrowed TracingData (data == NULL or n == 0
// drops it and every vector behind it).  The particle models index it by the primitive id of the caller's geometry.
int vr_set_global_data(vr_context *c, uint32_t vecIdx, const float *data, uint32_t n) {
  if (!c || vecIdx >= 16 || (n && !data))
    return fail(c, VR_E_INVALID, "vr_set_global_data: bad argument (at most 16 vectors)");
  if (!data || n == 0) {
    drop_global_from(c, vecIdx);
  } else {
    if (c->globalVecs.size() <= vecIdx)
      c->globalVecs.resize(vecIdx + 1);
    c->globalRows.resize(c->globalVecs.size());
    c->globalVecs[vecIdx].assign(data, data + n);
    c->globalRows[vecIdx].len = n;
    c->globalRows[vecIdx].onDevice = false;
    c->globalRows[vecIdx].pending = true;
  }
  c->globalDirty = true;
  c->prepared = false;
  return VR_OK;
}
// vr_set_global_data for a vector that lives on the device.  The row is written where the kernels read it, now: one
// kernel copies the vector into its row of dGlobalVec (zeros up to the stride).  The rows have to move for a longer
// vector than any before, or more vectors than before.
int vr_set_global_data_device(vr_context *c, uint32_t vecIdx, const float *data, uint32_t n, void *stream) {
  if (!c || vecIdx >= 16)
    return fail(c, VR_E_INVALID, "vr_set_global_data_device: bad argument (at most 16 vectors)");
  if (!data || n == 0) { // (the rows that stay are where they were: nothing to upload)
    drop_global_from(c, vecIdx);
    c->prepared = false;
    return VR_OK;
  }
  VR_TRY(hand_over(c, {data}, "vr_set_global_data_device: data is not device memory of the context's device", stream));
  c->globalRows.resize(c->globalVecs.size());
  const uint32_t rows = std::max<uint32_t>((uint32_t)c->globalVecs.size(), vecIdx + 1);
  VR_TRY(lay_global_rows(c, rows, n)); // (an error leaves the vectors as they were)
  VR_HIP(c, launch_global_row(data, n, c->dGlobalVec.p + (size_t)vecIdx * c->globalStride, c->globalStride, c->stream));
  VR_TRY(caller_waits(c, stream));
  for (uint32_t v = (uint32_t)c->globalVecs.size(); v < rows; ++v) { // (vectors in between that were never given: empty,
    c->globalVecs.emplace_back();                                     //  and their rows are zero already)
    c->globalRows.emplace_back();
  }
  c->globalVecs[vecIdx].clear();
  c->globalRows[vecIdx].len = n;
  c->globalRows[vecIdx].onDevice = true;
  c->globalRows[vecIdx].pending = false;
  c->prepared = false; // (the launch parameters carry the row count and the stride)
  return VR_OK;
}
int vr_set_global_scalars(vr_context *c, const float *data, uint32_t n) {
  if (!c || (n && !data))
    return fail(c, VR_E_INVALID, "vr_set_global_scalars: bad argument");
  c->globalScalars.assign(data, data + n);
  c->globalDirty = true;
  c->prepared = false;
  return VR_OK;
}
// flux statistics: two companion planes per particle behind its data labels (vr_context::fluxStats).  The planes of the
// accumulator array move: the last result and a bound buffer of the other size do not survive the switch.
int vr_set_flux_statistics(vr_context *c, int on) {
  if (!c)
    return VR_E_INVALID;
  if (c->fluxStats == (on != 0))
    return VR_OK;
  c->fluxStats = on != 0;
  if (c->boundFlux && c->boundFluxN != c->geo.numPrims * c->totalPlanes()) {
    c->boundFlux = nullptr;
    c->boundFluxN = 0;
  }
  c->prepared = false;
  c->launched = false;
  c->haveResult = false;
  return VR_OK;
}
int vr_set_use_wdist(vr_context *c, int on) {
  if (!c)
    return VR_E_INVALID;
  c->useWdist = on != 0;
  c->prepared = false;
  return VR_OK;
}
// Source::getSourceArea() (raySource.hpp:17) of a user source, used by normalizeFlux(SOURCE)
// (rayTraceDisk.hpp:127); area <= 0 restores SourceRandom's (the source face of the bounding box).  Independent of the
// source in force: no source setter touches it (a surface source's own area goes first while one is in force)
int vr_set_source_area(vr_context *c, float area) {
  if (!c)
    return VR_E_INVALID;
  c->sourceAreaOverride = area > 0.f ? area : 0.f;
  return VR_OK;
}
// apply() is called once per time step with a ray count that follows the surface: reserve the ray-stream
// buffers for the largest count expected (they also grow by half again on their own and are kept)
int vr_reserve_rays(vr_context *c, uint64_t n) {
  if (!c)
    return VR_E_INVALID;
  c->reserveRays = n;
  c->prepared = false;
  return VR_OK;
}
int vr_set_number_of_rays_per_point(vr_context *c, uint64_t n) {
  if (!c)
    return VR_E_INVALID;
  c->numRaysPerPoint = n;
  c->numRaysFixed = 0;
  return VR_OK;
}
int vr_set_number_of_rays_fixed(vr_context *c, uint64_t n) {
  if (!c)
    return VR_E_INVALID;
  c->numRaysFixed = n;
  c->numRaysPerPoint = 0;
  return VR_OK;
}
int vr_set_max_reflections(vr_context *c, uint32_t n) {
  if (!c)
    return VR_E_INVALID;
  c->maxReflections = n;
  return VR_OK;
}
int vr_set_max_boundary_hits(vr_context *c, uint32_t n) {
  if (!c)
    return VR_E_INVALID;
  c->maxBoundaryHits = n;
  return VR_OK;
}
int vr_set_rng_seed(vr_context *c, uint32_t s) {
  if (!c)
    return VR_E_INVALID;
  c->rngSeed = s;
  c->useRandomSeed = false;
  return VR_OK;
}
int vr_set_use_random_seeds(vr_context *c, int b) {
  if (!c)
    return VR_E_INVALID;
  c->useRandomSeed = b != 0;
  return VR_OK;
}
int vr_set_run_number(vr_context *c, uint32_t r) {
  if (!c)
    return VR_E_INVALID;
  c->runNumber = r;
  return VR_OK;
}
int vr_set_world_size(vr_context *c, uint32_t world) {
  if (!c || world == 0 || world > (1u << 20))
    return fail(c, VR_E_INVALID, "vr_set_world_size: 1 .. 2^20 ranks");
  c->worldSize = world;
  return VR_OK;
}

int vr_set_ray_range(vr_context *c, uint64_t first, uint64_t count) {
  if (!c)
    return VR_E_INVALID;
  c->rayFirst = first;
  c->rayCount = count;
  return VR_OK;
}

int vr_set_data_log_shape(vr_context *c, const uint32_t *rowSizes, uint32_t rows) {
  if (!c || (rows && !rowSizes))
    return fail(c, VR_E_INVALID, "vr_set_data_log_shape: bad argument");
  if (rows > (uint32_t)VR_LOG_MAX_ROWS)
    return fail(c, VR_E_INVALID, "vr_set_data_log_shape: at most 16 rows");
  uint64_t total = 0;
  for (uint32_t r = 0; r < rows; ++r)
    total += rowSizes[r];
  if (total > VR_LOG_MAX_ENTRIES)
    return fail(c, VR_E_INVALID, "vr_set_data_log_shape: at most 65536 entries in all rows together");
  c->logRowSizes.assign(rowSizes, rowSizes + rows);
  c->logTotal = (uint32_t)total;
  c->logActive = false;
  c->haveLog = false;
  c->prepared = false; // (a prepared launch carries the old shape in its frame)
  return VR_OK;
}

void *vr_stream(vr_context *c) { return c ? (void *)c->stream : nullptr; }

int vr_get_run_number(const vr_context *c, uint32_t *out) {
  if (!c || !out)
    return VR_E_INVALID;
  *out = c->runNumber;
  return VR_OK;
}

} // extern "C"
