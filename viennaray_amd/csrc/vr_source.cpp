// vr_source.cpp — the source entry points of the C ABI: the seven vr_set_* calls that put a ray source in force or take
// one back.  Each does everything that can fail — argument checks, uploads, the device-side validation — and then ends in
// one call of RaySource (vr_source.hpp), which holds the transition and the table of the clearing calls.
#include <cmath>
#include <string>

#include "vr_context.hpp"

namespace vr {

// ---- messages that the host setter of a surface source and its device twin share -----
// (on purpose under the host setter's name: the device twin applies the host loop's checks and reports what it would)
static const char kSurfaceNullError[] =
    "vr_set_surface_source: positions, normals and weights must not be NULL when n > 0";
// the per-row refusals of a surface source, in the order they are checked: 0 position, 1 normal, 2 weight
static std::string surface_row_error(int kind, uint64_t row) {
  const std::string j = std::to_string(row);
  return kind == 0   ? "vr_set_surface_source: position " + j + " is not finite"
         : kind == 1 ? "vr_set_surface_source: normal " + j + " has zero or non-finite length"
                     : "vr_set_surface_source: weight " + j + " is negative or not finite";
}
// ... and of its scalars (nullptr: accepted)
static const char *surface_scalar_error(float sourceArea, float sourceOffset) {
  if (!(sourceArea > 0.f) || !std::isfinite(sourceArea))
    return "vr_set_surface_source: sourceArea must be positive and finite";
  if (!(sourceOffset >= 0.f) || !std::isfinite(sourceOffset))
    return "vr_set_surface_source: sourceOffset must be finite and >= 0";
  return nullptr;
}

} // namespace vr

extern "C" {

// Source = SourceGrid(points, particle's cosine power) (raySourceGrid.hpp); n == 0: back to SourceRandom
int vr_set_source_grid(vr_context *c, const float *points3, uint32_t n) {
  if (!c || (n && !points3))
    return fail(c, VR_E_INVALID, "vr_set_source_grid: bad argument");
  c->src.set_grid(points3, n);
  c->prepared = false;
  return VR_OK;
}
// Rays of a host-side Source callback for the NEXT applies: ray idx starts at org3[3 idx] towards
// dir3[3 idx] having consumed draws[idx] outputs of its engine (NULL: none).  n == 0: back to SourceRandom.
int vr_set_host_rays(vr_context *c, const float *org3, const float *dir3, const uint32_t *draws, uint64_t n) {
  if (!c || (n && (!org3 || !dir3)) || n > 0xFFFFFFFFull)
    return fail(c, VR_E_INVALID, "vr_set_host_rays: bad argument");
  c->src.set_host_rays(org3, dir3, draws, n);
  c->prepared = false;
  return VR_OK;
}
// Source model (vr_register_source_model): the next applies sample their rays on the device with model `sourceId`
// (< 0: back to SourceRandom if a model is in force), which reads params[0 .. nparams) (at most 16; zeros behind them) and
// the table — ntable floats, copied to the device here (NULL or 0: none).  numRays == 0: the ray count is SourceRandom's
// (numRaysFixed, or numRaysPerPoint per primitive); > 0: the source's own (at most 2^32 - 1, as for host rays).  It takes
// the place of a source grid, host rays and a surface source, and each of those takes its place; vr_set_source_area keeps
// supplying getSourceArea().  A refused call leaves the source in force as it was.
int vr_set_source_model(vr_context *c, int32_t sourceId, const float *params, uint32_t nparams, const float *table,
                        uint32_t ntable, uint64_t numRays) {
  if (!c)
    return VR_E_INVALID;
  if (sourceId < 0) {
    if (c->src.clear_if(SourceKind::Model))
      c->prepared = false;
    return VR_OK;
  }
  if ((size_t)sourceId >= c->sourceModels.size())
    return fail(c, VR_E_INVALID, "vr_set_source_model: unknown source model id (vr_register_source_model returns it)");
  if (nparams > (uint32_t)VR_SOURCE_PARAMS || (nparams && !params))
    return fail(c, VR_E_INVALID, "vr_set_source_model: at most 16 parameters (and params must not be NULL when nparams > 0)");
  if (numRays > 0xFFFFFFFFull)
    return fail(c, VR_E_INVALID, "vr_set_source_model: at most 2^32 - 1 rays");
  const bool haveTable = table && ntable;
  if (haveTable) {
    VR_HIP(c, hipSetDevice(c->device));
    VR_HIP(c, hipStreamSynchronize(c->stream)); // (a launched apply may still read the previous table)
    VR_HIP(c, c->dSrcTable.upload(table, ntable));
  }
  c->src.set_model(sourceId, c->sourceModels[sourceId].hasWeight, params, nparams, haveTable ? ntable : 0, numRays);
  c->prepared = false;
  return VR_OK;
}
// The table of the source model in force, from device memory: copied into the library's own buffer on the context's
// stream behind what `stream` holds now, and `stream` then waits for the copy (the ordering contract of
// vr_set_global_data_device: the caller may reuse its buffer in the order of its stream).  The copy runs behind an apply
// launched earlier.  ntable == 0 drops the table.  Refused — no source model in force, dTable not device memory of the
// context's device — the previous table stays.
int vr_set_source_model_table_device(vr_context *c, const float *dTable, uint32_t ntable, void *stream) {
  if (!c)
    return VR_E_INVALID;
  if (c->src.kind != SourceKind::Model)
    return fail(c, VR_E_STATE, "vr_set_source_model_table_device: no source model is set (vr_set_source_model first)");
  if (!dTable || ntable == 0) {
    c->src.srcTableCount = 0;
    c->prepared = false;
    return VR_OK;
  }
  VR_TRY(hand_over(c, {dTable}, "vr_set_source_model_table_device: the table is not device memory of the context's device", stream));
  if (!c->dSrcTable.holds(ntable)) { // (the buffer has to move: only once nothing reads the old one)
    VR_TRY(host_waits(c));
    VR_HIP(c, c->dSrcTable.ensure(ntable));
  }
  VR_HIP(c, hipMemcpyAsync(c->dSrcTable.p, dTable, (size_t)ntable * 4, hipMemcpyDeviceToDevice, c->stream));
  VR_TRY(caller_waits(c, stream));
  c->src.srcTableCount = ntable;
  c->prepared = false;
  return VR_OK;
}
// Surface source (gpu/raygTrace.hpp:267-297 setSurfaceSource / clearSurfaceSource): the next applies start their rays ON
// the n points — numRaysFixed if set, else numRaysPerPoint, rays each (:134-149) — from positions3[3 j] + unit normal *
// sourceOffset along a cosine distribution about normals3[3 j] (any non-zero length), with start weight weights[j];
// normalizeFlux(SOURCE) then uses sourceArea (gpu/raygTraceDisk.hpp:90-91).  n == 0: back to SourceRandom if a surface
// source is in force.
int vr_set_surface_source(vr_context *c, const float *positions3, const float *normals3, const float *weights, uint32_t n,
                          float sourceArea, float sourceOffset) {
  if (!c)
    return VR_E_INVALID;
  if (n == 0) {
    if (c->src.clear_if(SourceKind::Surface))
      c->prepared = false;
    return VR_OK;
  }
  if (!positions3 || !normals3 || !weights)
    return fail(c, VR_E_INVALID, kSurfaceNullError);
  if (const char *msg = surface_scalar_error(sourceArea, sourceOffset))
    return fail(c, VR_E_INVALID, msg);
  for (size_t j = 0; j < n; ++j) {
    const float *q = positions3 + 3 * j, *m = normals3 + 3 * j;
    if (!std::isfinite(q[0]) || !std::isfinite(q[1]) || !std::isfinite(q[2]))
      return fail(c, VR_E_INVALID, surface_row_error(0, j).c_str());
    const float len = std::sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]); // (as the generator's vnormalize)
    if (!(len > 0.f) || !std::isfinite(len))
      return fail(c, VR_E_INVALID, surface_row_error(1, j).c_str());
    if (!(weights[j] >= 0.f) || !std::isfinite(weights[j]))
      return fail(c, VR_E_INVALID, surface_row_error(2, j).c_str());
  }
  VR_HIP(c, hipSetDevice(c->device));
  VR_HIP(c, hipStreamSynchronize(c->stream)); // (a launched apply may still read the previous tables)
  VR_HIP(c, c->dSurfPos.ensure((size_t)n * 3));
  VR_HIP(c, c->dSurfNrm.ensure((size_t)n * 3));
  VR_HIP(c, c->dSurfWeights.ensure(n));
  VR_HIP(c, hipMemcpy(c->dSurfPos.p, positions3, (size_t)n * 12, hipMemcpyHostToDevice));
  VR_HIP(c, hipMemcpy(c->dSurfNrm.p, normals3, (size_t)n * 12, hipMemcpyHostToDevice));
  VR_HIP(c, hipMemcpy(c->dSurfWeights.p, weights, (size_t)n * 4, hipMemcpyHostToDevice));
  c->src.set_surface(n, sourceArea, sourceOffset);
  c->prepared = false;
  return VR_OK;
}
// vr_set_surface_source for tables that live on the device (rows of ld = 2 or 3 floats; 2 only on a 2-D context, the
// third column then reads 0).  One kernel packs the rows into staging tables and applies the host loop's three checks to
// every row; one word comes back: the first refusal the host loop would have met, or none.  Accepted, the staging tables
// are swapped in; refused, the previous source stays untouched.
int vr_set_surface_source_device(vr_context *c, const float *positions, const float *normals, const float *weights,
                                 uint32_t n, uint32_t ld, float sourceArea, float sourceOffset, void *stream) {
  if (!c)
    return VR_E_INVALID;
  if (n == 0)
    return vr_set_surface_source(c, nullptr, nullptr, nullptr, 0, 0.f, 0.f);
  if (!positions || !normals || !weights)
    return fail(c, VR_E_INVALID, kSurfaceNullError);
  if (ld != 2 && ld != 3)
    return fail(c, VR_E_INVALID, "vr_set_surface_source_device: ld (floats per row) must be 2 or 3");
  if (ld == 2 && c->geo.D != 2)
    return fail(c, VR_E_INVALID, "vr_set_surface_source_device: rows of 2 floats need a 2-D geometry (D == 2)");
  if (const char *msg = surface_scalar_error(sourceArea, sourceOffset))
    return fail(c, VR_E_INVALID, msg);
  VR_TRY(hand_over(c, {positions, normals, weights},
                   "vr_set_surface_source_device: positions / normals / weights are not device memory of the context's "
                   "device",
                   stream));
  VR_HIP(c, c->dSurfPosIn.ensure((size_t)n * 3));
  VR_HIP(c, c->dSurfNrmIn.ensure((size_t)n * 3));
  VR_HIP(c, c->dSurfWeightsIn.ensure(n));
  VR_HIP(c, c->dSurfBad.ensure(1));
  VR_HIP(c, launch_surface_source(positions, normals, weights, n, ld, c->dSurfPosIn.p, c->dSurfNrmIn.p, c->dSurfWeightsIn.p,
                                  c->dSurfBad.p, c->stream));
  unsigned long long bad = 0;
  VR_HIP(c, hipMemcpyAsync(&bad, c->dSurfBad.p, sizeof(bad), hipMemcpyDeviceToHost, c->stream));
  VR_TRY(host_waits(c));
  if (bad != ~0ull)
    return fail(c, VR_E_INVALID, surface_row_error((int)(bad & 3ull), bad >> 2).c_str());
  std::swap(c->dSurfPos, c->dSurfPosIn);
  std::swap(c->dSurfNrm, c->dSurfNrmIn);
  std::swap(c->dSurfWeights, c->dSurfWeightsIn);
  c->src.set_surface(n, sourceArea, sourceOffset);
  c->prepared = false;
  return VR_OK;
}
// Source::getInitialRayWeight(idx) (raySource.hpp:18, rayTraceKernel.hpp:124) of the rays handed over with
// vr_set_host_rays: the weight a ray starts with and the scale of the roulette's thresholds.  n == 0: all 1.
int vr_set_host_ray_weights(vr_context *c, const float *weights, uint64_t n) {
  if (!c || (n && !weights))
    return fail(c, VR_E_INVALID, "vr_set_host_ray_weights: bad argument");
  if (!c->src.set_host_weights(weights, n))
    return fail(c, VR_E_INVALID, "vr_set_host_ray_weights: one weight per host ray (call vr_set_host_rays first)");
  c->prepared = false;
  return VR_OK;
}

} // extern "C"
