// vr_results.cpp — what an apply() left behind: flux, TraceInfo and the data log; normalizeFlux / smoothFlux; areas,
// bounding box and neighbour counts of the geometry; per-primitive values mapped to the caller's points.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "vr_context.hpp"
#include "vr_frame.hpp"

static_assert(VR_LOG_SCALE == (double)(1ull << VR_LOG_FRAC_BITS), "the kernels' log scale is 2^VR_LOG_FRAC_BITS");

// Source::getSourceArea(): a surface source's own (gpu/raygTraceDisk.hpp:90-91), a user source's override, else
// SourceRandom's — the source face of the bounding box
static float effective_source_area(const vr_context *c) {
  if (c->src.kind == SourceKind::Surface)
    return c->src.surfArea;
  return c->sourceAreaOverride > 0.f ? c->sourceAreaOverride : c->sourceArea;
}

extern "C" {

// ---- results --------------------------------------------------------------------
uint32_t vr_num_primitives(const vr_context *c) { return c ? c->geo.numPrims : 0; }

uint32_t vr_num_data(const vr_context *c) { return c ? c->totalData : 0; }

static int get_flux_plane_f64(vr_context *c, uint32_t dataIdx, double *out, uint32_t n);

int vr_get_flux_f64(vr_context *c, double *out, uint32_t n) { return get_flux_plane_f64(c, 0, out, n); }

// getLocalData().getVectorData(dataIdx): the particle's data label `dataIdx`, as the reference's float vector.
// The int64 fixed-point sums become floats on the device (float(double(acc) * 2^-40), what the host conversion
// did): one 4-byte-per-primitive download instead of 8 bytes and two host passes.
int vr_get_flux_data(vr_context *c, uint32_t dataIdx, float *out, uint32_t n) {
  if (!c || !out)
    return VR_E_INVALID;
  if (!c->haveResult)
    return fail(c, VR_E_STATE, "vr_get_flux: no result (call vr_apply)");
  if (n != c->geo.numPrims)
    return fail(c, VR_E_INVALID, "vr_get_flux: size mismatch");
  if (dataIdx >= c->totalData)
    return fail(c, VR_E_INVALID, "vr_get_flux_data: the particle has no such data label");
  VR_HIP(c, hipSetDevice(c->device));
  VR_HIP(c, c->dFluxTmp.ensure(n));
  VR_HIP(c, launch_flux_from_acc(c->fluxOut() + (size_t)c->planeOfData(dataIdx) * n, n, c->dFluxTmp.p, c->stream));
  VR_HIP(c, hipMemcpyAsync(out, c->dFluxTmp.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  VR_HIP(c, hipStreamSynchronize(c->stream));
  return VR_OK;
}

static int get_flux_plane_f64(vr_context *c, uint32_t dataIdx, double *out, uint32_t n) {
  if (!c || !out)
    return VR_E_INVALID;
  if (!c->haveResult)
    return fail(c, VR_E_STATE, "vr_get_flux: no result (call vr_apply)");
  if (n != c->geo.numPrims)
    return fail(c, VR_E_INVALID, "vr_get_flux: size mismatch");
  if (dataIdx >= c->totalData)
    return fail(c, VR_E_INVALID, "vr_get_flux_data: the particle has no such data label");
  VR_HIP(c, hipSetDevice(c->device));
  std::vector<unsigned long long> acc(n);
  VR_HIP(c, hipMemcpy(acc.data(), c->fluxOut() + (size_t)c->planeOfData(dataIdx) * n, (size_t)n * 8, hipMemcpyDeviceToHost));
  const double scale = std::ldexp(1.0, -VR_FLUX_FRAC_BITS);
  for (uint32_t i = 0; i < n; ++i)
    out[i] = (double)acc[i] * scale;
  return VR_OK;
}

int vr_get_flux(vr_context *c, float *out, uint32_t n) { return vr_get_flux_data(c, 0, out, n); }

int vr_get_trace_info(const vr_context *c, vr_trace_info *out) {
  if (!c || !out)
    return VR_E_INVALID;
  *out = c->info;
  return VR_OK;
}

int vr_get_particle_trace_info(const vr_context *c, uint32_t q, vr_trace_info *out) {
  if (!c || !out)
    return VR_E_INVALID;
  if (c->specs.size() <= 1) {
    if (q != 0)
      return VR_E_INVALID;
    *out = c->info;
    return VR_OK;
  }
  if (q >= c->launches.size())
    return VR_E_INVALID;
  *out = c->launches[q].info;
  return VR_OK;
}

int vr_get_trace_mode(const vr_context *c, int32_t *mode) {
  if (!c || !mode)
    return VR_E_INVALID;
  *mode = c->launches.empty() ? 0 : current_launch(c).traceMode;
  return VR_OK;
}

int vr_flux_accumulators(vr_context *c, void **devPtr, uint32_t *n) {
  if (!c || !devPtr)
    return VR_E_INVALID;
  if (!c->haveResult)
    return fail(c, VR_E_STATE, "vr_flux_accumulators: no result");
  *devPtr = c->fluxOut();
  if (n)
    *n = c->geo.numPrims * c->totalPlanes();
  return VR_OK;
}

// ---- the data log (DataLog / logData of the reference: rayTraceKernel.hpp:131-133, 345) ---------------------------
int vr_get_data_log(vr_context *c, float *out, uint32_t n) {
  if (!c || (n && !out))
    return VR_E_INVALID;
  if (!c->haveLog)
    return fail(c, VR_E_STATE, "vr_get_data_log: no result (set a shape with vr_set_data_log_shape, then vr_apply)");
  if (n != c->logHost.size() - 1)
    return fail(c, VR_E_INVALID, "vr_get_data_log: n differs from the entries of the shape");
  const double scale = std::ldexp(1.0, -VR_LOG_FRAC_BITS);
  for (uint32_t i = 0; i < n; ++i)
    out[i] = (float)((double)(long long)c->logHost[i] * scale);
  return VR_OK;
}

int vr_get_data_log_i64(vr_context *c, int64_t *out, uint32_t n) {
  if (!c || (n && !out))
    return VR_E_INVALID;
  if (!c->haveLog)
    return fail(c, VR_E_STATE, "vr_get_data_log_i64: no result (set a shape with vr_set_data_log_shape, then vr_apply)");
  if (n != c->logHost.size() - 1)
    return fail(c, VR_E_INVALID, "vr_get_data_log_i64: n differs from the entries of the shape");
  for (uint32_t i = 0; i < n; ++i)
    out[i] = (int64_t)c->logHost[i];
  return VR_OK;
}

int vr_get_data_log_dropped(vr_context *c, uint64_t *out) {
  if (!c || !out)
    return VR_E_INVALID;
  if (!c->haveLog)
    return fail(c, VR_E_STATE, "vr_get_data_log_dropped: no result (set a shape with vr_set_data_log_shape, then vr_apply)");
  *out = c->logHost.back();
  return VR_OK;
}

int vr_data_log_accumulators(vr_context *c, void **devPtr, uint32_t *n) {
  if (!c || !devPtr || !n)
    return VR_E_INVALID;
  if (!c->logActive || !c->dDataLog.p)
    return fail(c, VR_E_STATE, "vr_data_log_accumulators: no data log (set a shape with vr_set_data_log_shape, then prepare or apply)");
  *devPtr = c->dDataLog.p;
  *n = c->logTotal;
  return VR_OK;
}

int vr_bind_flux_accumulators(vr_context *c, void *devPtr, uint32_t n) {
  if (!c)
    return VR_E_INVALID;
  if (devPtr && n != c->geo.numPrims * c->totalPlanes())
    return fail(c, VR_E_INVALID, "vr_bind_flux_accumulators: size mismatch (numPrims x data labels; set geometry and particle first)");
  c->boundFlux = (unsigned long long *)devPtr;
  c->boundFluxN = devPtr ? n : 0;
  return VR_OK;
}

// normalizeFlux on the device (rayTraceDisk.hpp:103-142, rayTraceTriangle.hpp:92-130;
// gpu/kernels/normKernels.cu:58-74): `flux` (device) holds the flux in the caller's order
static int normalize_on_device(vr_context *c, float *flux, uint32_t n, int normType) {
  const bool disk = c->geo.geo == 0;
  if (!c->areasValid)
    return fail(c, VR_E_STATE, "vr_normalize_flux: call vr_apply first (primitive areas)");
  float normFactor = 0.f;
  if (normType == VR_NORM_SOURCE) {
    if (c->numRaysLast == 0)
      return fail(c, VR_E_STATE, "No source was specified in rayTrace for the normalization.");
    normFactor = effective_source_area(c) / c->numRaysLast;
  } else if (normType != VR_NORM_MAX) {
    return VR_OK; // `default: break;` in the reference
  }
  const double totalDiskArea = c->geo.diskRadius * c->geo.diskRadius * M_PI;
  VR_HIP(c, c->dNormMax.ensure(1)); // (a word of its own: the builder's scratch does not exist under VR_HOST_BUILD)
  VR_HIP(c, launch_normalize_flux(flux, c->dAreas.p, n, disk ? 0 : 1, normType, normFactor, totalDiskArea,
                                  c->dNormMax.p, c->stream));
  return VR_OK;
}

int vr_normalize_flux(vr_context *c, float *flux, uint32_t n, int normType) {
  if (!c || !flux || n != c->geo.numPrims)
    return fail(c, VR_E_INVALID, "vr_normalize_flux: bad argument");
  VR_HIP(c, hipSetDevice(c->device));
  VR_HIP(c, c->dFluxTmp.ensure(n));
  VR_HIP(c, hipMemcpyAsync(c->dFluxTmp.p, flux, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  int r = normalize_on_device(c, c->dFluxTmp.p, n, normType);
  if (r != VR_OK)
    return r;
  VR_HIP(c, hipMemcpyAsync(flux, c->dFluxTmp.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  VR_HIP(c, hipStreamSynchronize(c->stream));
  return VR_OK;
}

// getLocalData().getVectorData(0) followed by normalizeFlux, without the raw flux ever
// visiting the host: int64 accumulators -> float -> normalised, one download
int vr_get_flux_normalized(vr_context *c, float *out, uint32_t n, int normType) {
  if (!c || !out)
    return VR_E_INVALID;
  if (!c->haveResult)
    return fail(c, VR_E_STATE, "vr_get_flux_normalized: no result (call vr_apply)");
  if (n != c->geo.numPrims)
    return fail(c, VR_E_INVALID, "vr_get_flux_normalized: size mismatch");
  VR_HIP(c, hipSetDevice(c->device));
  VR_HIP(c, c->dFluxTmp.ensure(n));
  VR_HIP(c, launch_flux_from_acc(c->fluxOut(), n, c->dFluxTmp.p, c->stream));
  int r = normalize_on_device(c, c->dFluxTmp.p, n, normType);
  if (r != VR_OK)
    return r;
  VR_HIP(c, hipMemcpyAsync(out, c->dFluxTmp.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  VR_HIP(c, hipStreamSynchronize(c->stream));
  return VR_OK;
}

// rayTraceDisk.hpp:146-193 (triangle version is a no-op: rayTraceTriangle.hpp:134-136)
int vr_smooth_flux(vr_context *c, float *flux, uint32_t n, int numNeighbors) {
  if (!c || !flux || n != c->geo.numPrims)
    return fail(c, VR_E_INVALID, "vr_smooth_flux: bad argument");
  if (c->geo.geo != 0 || numNeighbors < 1)
    return VR_OK;
  // device path: the geometry's own neighbourhood (numNeighbors == 1, what every reference example asks for) is
  // resident with the device-built scene; a wider one (k > 1) is a range query of radius k * 2 r over the resident BVH,
  // fused with the averaging.  No download of any neighbourhood.
  if (c->haveSetup && !c->geometryDirty && !read_knobs().hostSmooth) {
    VR_HIP(c, hipSetDevice(c->device));
    DevBuf<float> dIn, dOut;
    DevBuf<uint32_t> dOv;
    VR_HIP(c, dIn.ensure(n));
    VR_HIP(c, dOut.ensure(n));
    VR_HIP(c, dOv.ensure(1));
    uint32_t ov = 0;
    VR_HIP(c, hipMemcpyAsync(dIn.p, flux, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    VR_HIP(c, hipMemsetAsync(dOv.p, 0, 4, c->stream));
    if (numNeighbors == 1)
      VR_HIP(c, launch_smooth_flux(dIn.p, dOut.p, c->dNormal3.p, c->dNbOff.p, c->dNbIds.p, c->dOrder.p,
                                   c->dLeafOfOrig.p, n, dOv.p, c->stream));
    else
      VR_HIP(c, launch_smooth_wide(dIn.p, dOut.p, c->dNormal3.p, c->lastSetup, numNeighbors * 2 * c->geo.diskRadius,
                                   dOv.p, c->stream));
    VR_HIP(c, hipMemcpyAsync(&ov, dOv.p, 4, hipMemcpyDeviceToHost, c->stream));
    VR_HIP(c, hipStreamSynchronize(c->stream));
    if (ov == 0) {
      VR_HIP(c, hipMemcpy(flux, dOut.p, (size_t)n * 4, hipMemcpyDeviceToHost));
      return VR_OK;
    } // (some neighbourhood longer than the kernel's buffer: host path below)
  }
  {
    const int r = ensure_host_geometry(c); // (the host path reads the normals, and the centres for k > 1)
    if (r != VR_OK)
      return r;
  }
  if (numNeighbors == 1) {
    int r = ensure_host_neighbors(c);
    if (r != VR_OK)
      return r;
  }
  const std::vector<uint32_t> *off = &c->geo.nbOff, *ids = &c->geo.nbIds;
  std::vector<uint32_t> woff, wids;
  if (numNeighbors != 1) {
    std::vector<float> pts((size_t)n * 3);
    for (uint32_t i = 0; i < n; ++i)
      std::memcpy(&pts[3 * (size_t)i], &c->geo.disk4[4 * (size_t)i], 12);
    host_neighbors(c->geo.D, pts.data(), n, numNeighbors * 2 * c->geo.diskRadius, c->geo.minC, woff, wids);
    off = &woff;
    ids = &wids;
  }
  std::vector<float> old(flux, flux + n);
  const float *nr = c->geo.normal3.data();
  for (uint32_t i = 0; i < n; ++i) {
    float vv = old[i];
    float sum = 1.f;
    for (uint32_t j = (*off)[i]; j < (*off)[i + 1]; ++j) {
      const uint32_t nb = (*ids)[j];
      const float w = (nr[3 * (size_t)i] * nr[3 * (size_t)nb] + nr[3 * (size_t)i + 1] * nr[3 * (size_t)nb + 1]) +
                      nr[3 * (size_t)i + 2] * nr[3 * (size_t)nb + 2];
      if (w > 0.f) {
        vv += old[nb] * w;
        sum += w;
      }
    }
    flux[i] = vv / sum;
  }
  return VR_OK;
}

// vr_get_flux_device in three parts, the first two shared with vr_get_flux_at_points_device: what it refuses before it
// touches anything ...
static int flux_device_refusal(vr_context *c, uint32_t dataIdx, uint32_t n) {
  if (!c->haveResult)
    return fail(c, VR_E_STATE, "vr_get_flux_device: no result (call vr_apply)");
  if (n != c->geo.numPrims)
    return fail(c, VR_E_INVALID, "vr_get_flux_device: size mismatch");
  if (dataIdx >= c->totalData)
    return fail(c, VR_E_INVALID, "vr_get_flux_device: the particle has no such data label");
  return VR_OK;
}

// ... its work, queued on the context's stream between the hand-over and its end (`out` is device memory) ...
static int flux_on_device(vr_context *c, uint32_t dataIdx, float *out, uint32_t n, int normType, int numNeighbors) {
  const bool smooth = c->geo.geo == 0 && numNeighbors >= 1;
  float *work = out;
  if (smooth) { // (the smoothing kernels read one buffer and write another)
    VR_HIP(c, c->dFluxTmp.ensure(n));
    work = c->dFluxTmp.p;
  }
  VR_HIP(c, launch_flux_from_acc(c->fluxOut() + (size_t)c->planeOfData(dataIdx) * n, n, work, c->stream));
  if (normType == VR_NORM_SOURCE || normType == VR_NORM_MAX)
    VR_TRY(normalize_on_device(c, work, n, normType));
  if (smooth) {
    bool done = false;
    if (c->haveSetup && !c->geometryDirty && !read_knobs().hostSmooth) {
      DevBuf<uint32_t> dOv;
      VR_HIP(c, dOv.ensure(1));
      uint32_t ov = 0;
      VR_HIP(c, hipMemsetAsync(dOv.p, 0, 4, c->stream));
      if (numNeighbors == 1)
        VR_HIP(c, launch_smooth_flux(work, out, c->dNormal3.p, c->dNbOff.p, c->dNbIds.p, c->dOrder.p, c->dLeafOfOrig.p, n,
                                     dOv.p, c->stream));
      else
        VR_HIP(c, launch_smooth_wide(work, out, c->dNormal3.p, c->lastSetup, numNeighbors * 2 * c->geo.diskRadius, dOv.p,
                                     c->stream));
      VR_HIP(c, hipMemcpyAsync(&ov, dOv.p, 4, hipMemcpyDeviceToHost, c->stream));
      VR_HIP(c, hipStreamSynchronize(c->stream));
      done = ov == 0;
    }
    if (!done) { // the one path through the host: vr_smooth_flux's own fallback, then up again
      std::vector<float> h(n);
      VR_HIP(c, hipMemcpyAsync(h.data(), work, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
      VR_HIP(c, hipStreamSynchronize(c->stream));
      VR_TRY(vr_smooth_flux(c, h.data(), n, numNeighbors));
      VR_HIP(c, hipMemcpy(out, h.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    }
  }
  return VR_OK;
}

// getLocalData().getVectorData(dataIdx) -> normalizeFlux -> smoothFlux with every stage on the device and the result left
// in the caller's device buffer: the kernels vr_get_flux_data / vr_normalize_flux / vr_smooth_flux run, on the same floats,
// so the result has their bits.  Without smoothing nothing comes back to the host and nothing waits; with smoothing one
// word does (the kernels' overflow flag, which decides on the host fallback).
int vr_get_flux_device(vr_context *c, uint32_t dataIdx, float *out, uint32_t n, int normType, int numNeighbors,
                       void *stream) {
  if (!c || !out)
    return VR_E_INVALID;
  VR_TRY(flux_device_refusal(c, dataIdx, n));
  // (the hand-over of the device setters, vr_api.cpp, the other way round: out may still be in use by work the caller
  //  queued before this call)
  VR_TRY(hand_over(c, {n ? out : nullptr}, "vr_get_flux_device: out is not device memory of the context's device", stream));
  VR_TRY(flux_on_device(c, dataIdx, out, n, normType, numNeighbors));
  return caller_waits(c, stream);
}

// ---- per-primitive values at the caller's points (include/viennaray_amd.h has the definition; vr_map.hip the walk) -----
// what every form refuses before it touches anything; `api`: the entry point's name
static int map_refusal(vr_context *c, const char *api, uint32_t n, uint32_t ld, float radius) {
  const std::string name = api;
  if (n != c->geo.numPrims)
    return fail(c, VR_E_INVALID, (name + ": size mismatch (n must be the number of primitives)").c_str());
  if (ld != 2 && ld != 3)
    return fail(c, VR_E_INVALID, (name + ": ld is 2 or 3 floats per row").c_str());
  if (ld == 2 && c->geo.D != 2)
    return fail(c, VR_E_INVALID, (name + ": rows of 2 floats need a 2-D scene").c_str());
  if (!(radius >= 0.f) || !std::isfinite(radius))
    return fail(c, VR_E_INVALID, (name + ": the radius must be finite and not negative").c_str());
  return VR_OK;
}
// the walk needs the device build of the geometry in force: its float4 nodes and packed records (kept for disks and
// triangles alike; the host builder, VR_HOST_BUILD, leaves none)
static int map_state_refusal(vr_context *c, const char *api) {
  if (!c->haveSetup || c->geometryDirty || c->knobs.hostBuild || c->geo.numPrims == 0)
    return fail(c, VR_E_STATE, (std::string(api) + ": no scene build is resident for the geometry in force (call vr_apply or "
                                                   "vr_apply_prepare after setting it)").c_str());
  return VR_OK;
}
// the kernels, on the context's stream: every pointer is device memory, the arguments have been accepted
static int map_on_device(vr_context *c, const float *values, const float *points, const float *normals, uint32_t m,
                         uint32_t ld, float radius, float *out) {
  const uint32_t *perm = nullptr;
  bool waited = false;
  // (beyond 2^31 queries the pairs alone would take 48 GiB: walked in the caller's order)
  if (m >= read_knobs().mapSortMin && m <= (1u << 31)) {
    const size_t tiles = ((size_t)m + 1023) / 1024;
    VR_TRY(map_grow(c, c->dMapKeysA, m, waited));
    VR_TRY(map_grow(c, c->dMapKeysB, m, waited));
    VR_TRY(map_grow(c, c->dMapValsA, m, waited));
    VR_TRY(map_grow(c, c->dMapValsB, m, waited));
    VR_TRY(map_grow(c, c->dMapSortTable, 256 * tiles, waited));
    VR_TRY(map_grow(c, c->dMapScanTmp, 2 * ((256 * tiles) / 2048 + 4) + 64, waited));
    VR_HIP(c, launch_map_keys(points, m, ld, c->geo.D, c->sceneLo, c->sceneHi, c->dMapKeysA.p, c->dMapValsA.p, c->stream));
    VR_HIP(c, launch_sort_pairs(c->dMapKeysA.p, c->dMapValsA.p, c->dMapKeysB.p, c->dMapValsB.p, m, c->dMapSortTable.p,
                                c->dMapScanTmp.p, c->stream));
    perm = c->dMapValsA.p;
  }
  unsigned long long *visits = nullptr;
#ifdef VR_DIAG
  VR_TRY(map_grow(c, c->dMapVisits, 1, waited));
  visits = c->dMapVisits.p;
  VR_HIP(c, hipMemsetAsync(visits, 0, 8, c->stream));
#endif
  VR_HIP(c, launch_map_points(c->lastSetup, values, points, normals, m, ld, radius, perm, out, visits, c->stream));
#ifdef VR_DIAG
  if (c->knobs.printLaunches) { // (the diagnostic build's figure, for tools/map_points_bench.py)
    unsigned long long v = 0;
    VR_HIP(c, hipMemcpyAsync(&v, visits, 8, hipMemcpyDeviceToHost, c->stream));
    VR_HIP(c, hipStreamSynchronize(c->stream));
    std::fprintf(stderr, "map_points: m=%u sorted=%d node visits per query %.2f\n", m, perm ? 1 : 0, (double)v / m);
  }
#endif
  return VR_OK;
}

int vr_map_to_points_device(vr_context *c, const float *values, uint32_t n, const float *points, const float *normals,
                            uint32_t m, uint32_t ld, float radius, float *out, void *stream) {
  if (!c)
    return VR_E_INVALID;
  VR_TRY(map_refusal(c, "vr_map_to_points_device", n, ld, radius));
  if (m == 0)
    return VR_OK;
  if (!values || !points || !out)
    return fail(c, VR_E_INVALID, "vr_map_to_points_device: values, points and out must not be null");
  VR_TRY(map_state_refusal(c, "vr_map_to_points_device"));
  VR_TRY(hand_over(c, {values, points, normals, out},
                   "vr_map_to_points_device: values, points, normals and out must be device memory of the context's device",
                   stream));
  VR_TRY(map_on_device(c, values, points, normals, m, ld, radius, out));
  return caller_waits(c, stream);
}

int vr_map_to_points(vr_context *c, const float *values, uint32_t n, const float *points3, const float *normals3,
                     uint32_t m, float radius, float *out) {
  if (!c)
    return VR_E_INVALID;
  VR_TRY(map_refusal(c, "vr_map_to_points", n, 3, radius));
  if (m == 0)
    return VR_OK;
  if (!values || !points3 || !out)
    return fail(c, VR_E_INVALID, "vr_map_to_points: values, points3 and out must not be null");
  VR_TRY(map_state_refusal(c, "vr_map_to_points"));
  VR_HIP(c, hipSetDevice(c->device));
  bool waited = false;
  VR_TRY(map_grow(c, c->dMapValues, n, waited));
  VR_TRY(map_grow(c, c->dMapPoints, (size_t)m * 3, waited));
  if (normals3)
    VR_TRY(map_grow(c, c->dMapNormals, (size_t)m * 3, waited));
  VR_TRY(map_grow(c, c->dMapOut, m, waited));
  VR_HIP(c, hipMemcpyAsync(c->dMapValues.p, values, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  VR_HIP(c, hipMemcpyAsync(c->dMapPoints.p, points3, (size_t)m * 12, hipMemcpyHostToDevice, c->stream));
  if (normals3)
    VR_HIP(c, hipMemcpyAsync(c->dMapNormals.p, normals3, (size_t)m * 12, hipMemcpyHostToDevice, c->stream));
  VR_TRY(map_on_device(c, c->dMapValues.p, c->dMapPoints.p, normals3 ? c->dMapNormals.p : nullptr, m, 3, radius,
                       c->dMapOut.p));
  VR_HIP(c, hipMemcpyAsync(out, c->dMapOut.p, (size_t)m * 4, hipMemcpyDeviceToHost, c->stream));
  VR_HIP(c, hipStreamSynchronize(c->stream));
  return VR_OK;
}

int vr_get_flux_at_points_device(vr_context *c, uint32_t dataIdx, int normType, int numNeighbors, const float *points,
                                 const float *normals, uint32_t m, uint32_t ld, float radius, float *out, void *stream) {
  if (!c)
    return VR_E_INVALID;
  const uint32_t n = c->geo.numPrims;
  VR_TRY(map_refusal(c, "vr_get_flux_at_points_device", n, ld, radius));
  VR_TRY(flux_device_refusal(c, dataIdx, n));
  if (m == 0)
    return VR_OK;
  if (!points || !out)
    return fail(c, VR_E_INVALID, "vr_get_flux_at_points_device: points and out must not be null");
  VR_TRY(map_state_refusal(c, "vr_get_flux_at_points_device"));
  VR_TRY(hand_over(c, {points, normals, out},
                   "vr_get_flux_at_points_device: points, normals and out must be device memory of the context's device",
                   stream));
  bool waited = false;
  VR_TRY(map_grow(c, c->dMapFlux, n, waited));
  VR_TRY(flux_on_device(c, dataIdx, c->dMapFlux.p, n, normType, numNeighbors));
  VR_TRY(map_on_device(c, c->dMapFlux.p, points, normals, m, ld, radius, out));
  return caller_waits(c, stream);
}

// ---- flux statistics (vr_set_flux_statistics) ------------------------------------------------------------------------
// the planes of particle q in fluxOut(): *flux its label 0, *sumsq and *hits its two companions
static int stats_planes(vr_context *c, const char *api, uint32_t q, const void *out, uint32_t n, unsigned long long **flux,
                        unsigned long long **sumsq, unsigned long long **hits) {
  if (!c || !out)
    return VR_E_INVALID;
  const std::string name = api;
  if (!c->fluxStats)
    return fail(c, VR_E_STATE, (name + ": flux statistics are off (vr_set_flux_statistics)").c_str());
  if (!c->haveResult)
    return fail(c, VR_E_STATE, (name + ": no result (call vr_apply with flux statistics on; after vr_apply_launch, vr_apply_finish)").c_str());
  if (n != c->geo.numPrims)
    return fail(c, VR_E_INVALID, (name + ": size mismatch (n must be the number of primitives)").c_str());
  if (q >= c->numParticles())
    return fail(c, VR_E_INVALID, (name + ": particleIdx is beyond the particle list").c_str());
  const uint32_t numData = c->specs.empty() ? 1u : c->specs[q].numData;
  *flux = c->fluxOut() + (size_t)c->planeBase(q) * n;
  *sumsq = *flux + (size_t)numData * n;
  *hits = *sumsq + n;
  return VR_OK;
}

int vr_get_hit_counts(vr_context *c, uint32_t q, uint64_t *out, uint32_t n) {
  unsigned long long *flux, *sumsq, *hits;
  VR_TRY(stats_planes(c, "vr_get_hit_counts", q, out, n, &flux, &sumsq, &hits));
  VR_HIP(c, hipSetDevice(c->device));
  VR_HIP(c, hipMemcpyAsync(out, hits, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
  VR_HIP(c, hipStreamSynchronize(c->stream));
  return VR_OK;
}

int vr_get_flux_sum_squares(vr_context *c, uint32_t q, double *out, uint32_t n) {
  unsigned long long *flux, *sumsq, *hits;
  VR_TRY(stats_planes(c, "vr_get_flux_sum_squares", q, out, n, &flux, &sumsq, &hits));
  VR_HIP(c, hipSetDevice(c->device));
  std::vector<unsigned long long> acc(n);
  VR_HIP(c, hipMemcpyAsync(acc.data(), sumsq, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
  VR_HIP(c, hipStreamSynchronize(c->stream));
  const double scale = std::ldexp(1.0, -VR_FLUX_FRAC_BITS);
  for (uint32_t i = 0; i < n; ++i)
    out[i] = (double)acc[i] * scale;
  return VR_OK;
}

int vr_get_flux_error(vr_context *c, uint32_t q, int kind, float *out, uint32_t n) {
  unsigned long long *flux, *sumsq, *hits;
  VR_TRY(stats_planes(c, "vr_get_flux_error", q, out, n, &flux, &sumsq, &hits));
  if (kind != 0 && kind != 1)
    return fail(c, VR_E_INVALID, "vr_get_flux_error: kind is 0 (relative) or 1 (absolute)");
  VR_HIP(c, hipSetDevice(c->device));
  VR_HIP(c, c->dFluxTmp.ensure(n));
  VR_HIP(c, launch_flux_error(flux, sumsq, n, (double)c->numRaysLast, kind, c->dFluxTmp.p, c->stream));
  VR_HIP(c, hipMemcpyAsync(out, c->dFluxTmp.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  VR_HIP(c, hipStreamSynchronize(c->stream));
  return VR_OK;
}

// ... into the caller's device buffer, ordered like vr_get_flux_device: no host copy, nothing waits on the host
int vr_get_flux_error_device(vr_context *c, uint32_t q, int kind, float *out, uint32_t n, void *stream) {
  unsigned long long *flux, *sumsq, *hits;
  VR_TRY(stats_planes(c, "vr_get_flux_error_device", q, out, n, &flux, &sumsq, &hits));
  if (kind != 0 && kind != 1)
    return fail(c, VR_E_INVALID, "vr_get_flux_error_device: kind is 0 (relative) or 1 (absolute)");
  VR_TRY(hand_over(c, {n ? out : nullptr}, "vr_get_flux_error_device: out is not device memory of the context's device", stream));
  VR_HIP(c, launch_flux_error(flux, sumsq, n, (double)c->numRaysLast, kind, out, c->stream));
  return caller_waits(c, stream);
}

int vr_get_disk_areas(vr_context *c, float *out, uint32_t n) {
  if (!c || !out || n != c->geo.numPrims || c->geo.geo != 0 || !c->areasValid)
    return fail(c, VR_E_STATE, "vr_get_disk_areas: not available");
  if (!c->diskAreasHostValid) {
    VR_HIP(c, hipSetDevice(c->device));
    c->diskAreas.resize(n);
    VR_HIP(c, hipStreamSynchronize(c->stream));
    VR_HIP(c, hipMemcpy(c->diskAreas.data(), c->dAreas.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    c->diskAreasHostValid = true;
  }
  std::memcpy(out, c->diskAreas.data(), (size_t)n * 4);
  return VR_OK;
}
int vr_get_bounding_box(vr_context *c, float *out6) {
  if (!c || !out6)
    return VR_E_INVALID;
  for (int k = 0; k < 3; ++k) {
    out6[k] = c->bbLo[k];
    out6[k + 3] = c->bbHi[k];
  }
  return VR_OK;
}
float vr_get_source_area(vr_context *c) {
  return c ? effective_source_area(c) : 0.f;
}
float vr_get_disk_radius(const vr_context *c) { return c ? c->geo.diskRadius : 0.f; }
int vr_get_neighbor_counts(vr_context *c, uint32_t *out, uint32_t n) {
  if (!c || !out || n != c->geo.numPrims)
    return VR_E_INVALID;
  int r = ensure_host_neighbors(c);
  if (r != VR_OK)
    return r;
  for (uint32_t i = 0; i < n; ++i)
    out[i] = c->geo.nbOff[i + 1] - c->geo.nbOff[i];
  return VR_OK;
}

} // extern "C"
