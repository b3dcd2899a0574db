// vr_radiosity_solve.cpp — vr_radiosity_links_device / vr_radiosity_solve* / vr_radiosity_direct_device /
// vr_debug_radiosity_links / vr_radiosity_free_links: the steady-state flux of a diffusely re-emitting species from a
// recorded link table (include/viennaray_amd.h has the definition; vr_gather.hip records the table with the gather's own
// sample loop, vr_radiosity.hip iterates over it, vr_radiosity.hpp has the arithmetic).  Like vr_gather_flux.cpp the
// calls prepare nothing and touch none of prepared / launched / haveResult.  The recording walks the resident scene and
// refuses what a gather refuses; a solve walks nothing: it needs a table whose stamp still describes the settings in
// force, and says which setting moved when it does not.
#include <cmath>
#include <string>

#include "vr_context.hpp"
#include "vr_radiosity.hpp"

namespace vr {

// iterations launched between two reads of their residual words: 1, 2, 4, ... up to this many.  A kernel whose
// predecessor already met the tolerance does nothing (vr_radiosity.hip), so the batch size cannot show in t or F
constexpr uint32_t RAD_BATCH_MAX = 32;
// the link stream of an iteration goes by plain loads: measured against non-temporal ones (DESIGN.md 8s has the A/B;
// same bits either way) they are level on small tables, 10 % ahead at 264 MB and 3 % behind at 1 GB
constexpr bool RAD_NONTEMPORAL = false;

static vr_context::RadiosityStamp radiosity_stamp_now(const vr_context *c, uint32_t samples, float cosinePower) {
  vr_context::RadiosityStamp s;
  s.build = c->bvhBuilds;
  s.numPrims = c->geo.numPrims;
  for (int k = 0; k < 3; ++k)
    s.bcs[k] = c->bcs[k];
  s.sourceDirection = c->sourceDirection;
  s.maxBoundaryHits = c->maxBoundaryHits;
  s.seed = c->rngSeed;
  s.samples = samples;
  s.cosinePower = cosinePower;
  return s;
}

// nullptr, or what the table was built from that no longer holds
static const char *radiosity_stale(const vr_context *c) {
  const vr_context::RadiosityStamp &s = c->radStamp;
  if (c->geometryDirty || s.build != c->bvhBuilds || s.numPrims != c->geo.numPrims)
    return "the geometry has been set or rebuilt";
  if (s.bcs[0] != c->bcs[0] || s.bcs[1] != c->bcs[1] || s.bcs[2] != c->bcs[2])
    return "the boundary conditions have changed";
  if (s.sourceDirection != c->sourceDirection)
    return "the source direction has changed";
  if (s.maxBoundaryHits != c->maxBoundaryHits)
    return "maxBoundaryHits has changed";
  if (s.seed != c->rngSeed)
    return "the rng seed has changed";
  return nullptr;
}

// what every call that reads the table refuses
static int radiosity_table_refusal(vr_context *c, const char *api) {
  const std::string name = api;
  if (!c->radValid)
    return fail(c, VR_E_STATE, (name + ": no link table is resident (call vr_radiosity_links_device)").c_str());
  if (const char *why = radiosity_stale(c))
    return fail(c, VR_E_STATE, (name + ": the link table no longer matches the settings in force: " + why +
                                " since vr_radiosity_links_device")
                                   .c_str());
  return VR_OK;
}

static int radiosity_solve_refusal(vr_context *c, const char *api, const float *reflectivity, float scalar, float tolerance,
                                   const void *out) {
  const std::string name = api;
  if (!(tolerance >= 0.f))
    return fail(c, VR_E_INVALID, (name + ": tolerance must not be negative or NaN").c_str());
  if (!reflectivity && !radiosity_rho_ok(scalar))
    return fail(c, VR_E_INVALID, (name + ": the reflectivity must lie in [0, 1]").c_str());
  if (!out)
    return fail(c, VR_E_INVALID, (name + ": out must not be null").c_str());
  return VR_OK;
}

// what a solve starts from, on the context's stream: the work buffers, rho (nullptr: the scalar) in leaf order and its
// verdict — ONE word back, the lowest index that is refused — F_0 and e_1, and the arguments every iteration shares
static int solve_begin(vr_context *c, const char *api, const float *rho, float scalar, float tolerance, RadiosityArgs &a) {
  const uint32_t n = c->radStamp.numPrims, samples = c->radStamp.samples;
  bool waited = false;
  VR_TRY(map_grow(c, c->dRadRho, n, waited));
  VR_TRY(map_grow(c, c->dRadF, n, waited));
  VR_TRY(map_grow(c, c->dRadE0, n, waited));
  VR_TRY(map_grow(c, c->dRadE1, n, waited));
  VR_TRY(map_grow(c, c->dRadWords, 1 + RAD_BATCH_MAX, waited));
  uint32_t *const bad = c->dRadWords.p;
  VR_HIP(c, hipMemsetAsync(bad, 0xFF, 4, c->stream));
  VR_HIP(c, launch_radiosity_rho(rho, scalar, c->dLeafOfOrig.p, n, c->dRadRho.p, bad, c->stream));
  if (rho) {
    uint32_t first = 0xFFFFFFFFu;
    VR_HIP(c, hipMemcpyAsync(&first, bad, 4, hipMemcpyDeviceToHost, c->stream));
    VR_TRY(host_waits(c));
    if (first != 0xFFFFFFFFu)
      return fail(c, VR_E_INVALID, (std::string(api) + ": reflectivity[" + std::to_string(first) +
                                    "] is NaN, negative or above 1 (the lowest such index)")
                                       .c_str());
  }
  VR_HIP(c, launch_radiosity_init(c->dRadDirect.p, c->dRadRho.p, n, samples, c->dRadF.p, c->dRadE0.p, c->stream));
  a = RadiosityArgs{};
  a.links = c->dRadLinks.p;
  a.direct = c->dRadDirect.p;
  a.rho = c->dRadRho.p;
  a.F = c->dRadF.p;
  a.tolerance = tolerance;
  a.n = n;
  a.samples = samples;
  a.slots = radiosity_slots(n);
  a.wmax = gather_wmax(samples);
  return VR_OK;
}

// the solve on the context's stream: rho (nullptr: the scalar) and out are device memory, the arguments and the table
// have been accepted.  The host waits: the verdict on rho and the residual words come back
static int solve_on_device(vr_context *c, const char *api, const float *rho, float scalar, float tolerance, uint32_t maxIterations,
                           float *out, uint32_t *iterations, float *residual) {
  RadiosityArgs a;
  VR_TRY(solve_begin(c, api, rho, scalar, tolerance, a));
  const uint32_t n = a.n;
  uint32_t *const words = c->dRadWords.p + 1;
  const bool nontemporal = RAD_NONTEMPORAL;
  float *const e[2] = {c->dRadE0.p, c->dRadE1.p};
  uint32_t t = 0, lastBits = 0, batch = 1;
  bool stopped = false;
  while (!stopped && t < maxIterations) {
    const uint32_t m = std::min(batch, maxIterations - t);
    uint32_t got[RAD_BATCH_MAX];
    VR_HIP(c, hipMemsetAsync(words, 0, (size_t)m * 4, c->stream));
    for (uint32_t k = 0; k < m; ++k) { // iteration t + k + 1 reads e_{t+k+1}, written by the one before it (or the init)
      a.eIn = e[(t + k) & 1u];
      a.eOut = e[(t + k + 1u) & 1u];
      a.residual = words + k;
      a.prevResidual = k ? words + k - 1 : nullptr;
      VR_HIP(c, launch_radiosity_iterate(a, nontemporal, c->stream));
    }
    VR_HIP(c, hipMemcpyAsync(got, words, (size_t)m * 4, hipMemcpyDeviceToHost, c->stream));
    VR_TRY(host_waits(c));
    for (uint32_t k = 0; k < m && !stopped; ++k) {
      ++t;
      lastBits = got[k];
      stopped = radiosity_stops(lastBits, tolerance); // (the kernels behind this one have done nothing)
    }
    batch = std::min(batch * 2u, RAD_BATCH_MAX);
  }
  VR_HIP(c, launch_radiosity_unpermute(c->dRadF.p, c->dLeafOfOrig.p, n, out, c->stream));
  if (iterations)
    *iterations = t;
  if (residual)
    *residual = t ? radiosity_residual_value(lastBits) : 0.f;
  return VR_OK;
}

} // namespace vr

extern "C" {

uint64_t vr_radiosity_link_bytes(const vr_context *c, uint32_t samples) {
  if (!c)
    return 0;
  return radiosity_link_count(c->geo.numPrims, samples) * 4u + (uint64_t)c->geo.numPrims * 8u;
}

int vr_radiosity_links_device(vr_context *c, uint32_t samples, float cosinePower, void *stream) {
  if (!c)
    return VR_E_INVALID;
  const char *api = "vr_radiosity_links_device";
  const uint32_t n = c->geo.numPrims;
  // (the gather's checks for the whole scene in NORMAL mode; there is no `out` here for them to find null)
  VR_TRY(gather_refusal(c, api, 0, n, samples, cosinePower, VR_GATHER_NORMAL, nullptr, c));
  VR_TRY(resident_scene_refusal(c, api, "gather from"));
  VR_TRY(hand_over(c, {}, "", stream));
  // the table is replaced: from here on the previous one is gone, whatever happens
  c->radValid = false;
  const uint64_t entries = radiosity_link_count(n, samples);
  if (!c->dRadLinks.holds(entries) || !c->dRadDirect.holds(n) || !c->dRadOrigOfLeaf.holds(n)) {
    VR_TRY(host_waits(c)); // (a buffer that moves: vr_api.cpp)
    hipError_t e = c->dRadLinks.ensure(entries);
    if (e == hipSuccess)
      e = c->dRadDirect.ensure(n);
    if (e == hipSuccess)
      e = c->dRadOrigOfLeaf.ensure(n);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      c->dRadLinks.release();
      return fail(c, VR_E_HIP, (std::string(api) + ": no room for a link table of " + std::to_string(vr_radiosity_link_bytes(c, samples)) +
                                " bytes (" + hipGetErrorString(e) + "); no table is resident now")
                                   .c_str());
    }
  }
  bool waited = false;
  TraceParams p;
  GatherArgs a;
  VR_TRY(gather_params(c, waited, p, a, 0, n, samples, cosinePower, VR_GATHER_NORMAL));
  a.leafOfOrig = nullptr; // the whole scene: in leaf order
  a.acc = c->dRadDirect.p;
  a.links = c->dRadLinks.p;
  a.linkSlots = radiosity_slots(n);
  VR_HIP(c, hipMemsetAsync(c->dRadDirect.p, 0, (size_t)n * 8, c->stream));
  const unsigned slabs = (unsigned)std::min<size_t>(c->walkStackWaves, 0xFFFFFFFFu);
  gather_cut_chunks(a, slabs);
  VR_HIP(c, launch_gather_samples(p, c->geo.geo, c->geo.D, a, slabs, c->stream));
  VR_HIP(c, launch_radiosity_orig_of_leaf(c->dLeafOfOrig.p, n, c->dRadOrigOfLeaf.p, c->stream));
  c->radStamp = radiosity_stamp_now(c, samples, cosinePower);
  c->radValid = true;
  return caller_waits(c, stream);
}

int vr_radiosity_resident(const vr_context *c, uint32_t samples, float cosinePower) {
  if (!c || !c->radValid || radiosity_stale(c))
    return 0;
  return c->radStamp.samples == samples && c->radStamp.cosinePower == cosinePower ? 1 : 0;
}

int vr_radiosity_solve_device(vr_context *c, const float *reflectivity, float reflectivityScalar, float tolerance,
                              uint32_t maxIterations, float *out, uint32_t *iterations, float *residual, void *stream) {
  if (!c)
    return VR_E_INVALID;
  const char *api = "vr_radiosity_solve_device";
  VR_TRY(radiosity_solve_refusal(c, api, reflectivity, reflectivityScalar, tolerance, out));
  VR_TRY(radiosity_table_refusal(c, api));
  VR_TRY(hand_over(c, {reflectivity, out}, "vr_radiosity_solve_device: reflectivity and out must be device memory of the context's device",
                   stream));
  VR_TRY(solve_on_device(c, api, reflectivity, reflectivityScalar, tolerance, maxIterations, out, iterations, residual));
  return caller_waits(c, stream);
}

int vr_radiosity_solve(vr_context *c, const float *reflectivity, float reflectivityScalar, float tolerance, uint32_t maxIterations,
                       float *out, uint32_t *iterations, float *residual) {
  if (!c)
    return VR_E_INVALID;
  const char *api = "vr_radiosity_solve";
  VR_TRY(radiosity_solve_refusal(c, api, reflectivity, reflectivityScalar, tolerance, out));
  VR_TRY(radiosity_table_refusal(c, api));
  VR_HIP(c, hipSetDevice(c->device));
  const uint32_t n = c->radStamp.numPrims;
  bool waited = false;
  VR_TRY(map_grow(c, c->dRadOut, n, waited));
  if (reflectivity) {
    VR_TRY(map_grow(c, c->dRadIn, n, waited));
    VR_HIP(c, hipMemcpyAsync(c->dRadIn.p, reflectivity, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  }
  VR_TRY(solve_on_device(c, api, reflectivity ? c->dRadIn.p : nullptr, reflectivityScalar, tolerance, maxIterations, c->dRadOut.p,
                         iterations, residual));
  VR_HIP(c, hipMemcpyAsync(out, c->dRadOut.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  VR_HIP(c, hipStreamSynchronize(c->stream));
  return VR_OK;
}

int vr_radiosity_direct_device(vr_context *c, float *out, void *stream) {
  if (!c)
    return VR_E_INVALID;
  const char *api = "vr_radiosity_direct_device";
  if (!out)
    return fail(c, VR_E_INVALID, "vr_radiosity_direct_device: out must not be null");
  VR_TRY(radiosity_table_refusal(c, api));
  VR_TRY(hand_over(c, {out}, "vr_radiosity_direct_device: out must be device memory of the context's device", stream));
  const uint32_t n = c->radStamp.numPrims;
  bool waited = false;
  VR_TRY(map_grow(c, c->dRadF, n, waited));
  VR_HIP(c, launch_gather_finish(c->dRadDirect.p, n, c->radStamp.samples, c->dRadF.p, c->stream));
  VR_HIP(c, launch_radiosity_unpermute(c->dRadF.p, c->dLeafOfOrig.p, n, out, c->stream));
  return caller_waits(c, stream);
}

int vr_debug_radiosity_links(vr_context *c, uint32_t prim, uint32_t first, uint32_t count, int32_t *links) {
  if (!c)
    return VR_E_INVALID;
  const char *api = "vr_debug_radiosity_links";
  VR_TRY(radiosity_table_refusal(c, api));
  if (prim >= c->radStamp.numPrims)
    return fail(c, VR_E_INVALID, "vr_debug_radiosity_links: prim is beyond vr_num_primitives");
  if ((uint64_t)first + count > c->radStamp.samples)
    return fail(c, VR_E_INVALID, "vr_debug_radiosity_links: first + count is beyond the table's samples");
  if (count && !links)
    return fail(c, VR_E_INVALID, "vr_debug_radiosity_links: links must not be null");
  if (count == 0)
    return VR_OK;
  VR_HIP(c, hipSetDevice(c->device));
  bool waited = false;
  VR_TRY(map_grow(c, c->dRadDebug, count, waited));
  VR_HIP(c, launch_radiosity_debug_links(c->dRadLinks.p, radiosity_slots(c->radStamp.numPrims), c->dLeafOfOrig.p, prim, first, count,
                                         c->dRadOrigOfLeaf.p, c->dRadDebug.p, c->stream));
  VR_HIP(c, hipMemcpyAsync(links, c->dRadDebug.p, (size_t)count * 4, hipMemcpyDeviceToHost, c->stream));
  VR_HIP(c, hipStreamSynchronize(c->stream));
  return VR_OK;
}

int vr_debug_radiosity_time_iterations(vr_context *c, float reflectivityScalar, uint32_t count, int nontemporal,
                                       float *msPerIteration) {
  if (!c)
    return VR_E_INVALID;
  const char *api = "vr_debug_radiosity_time_iterations";
  if (count == 0 || !msPerIteration)
    return fail(c, VR_E_INVALID, "vr_debug_radiosity_time_iterations: count must not be 0, msPerIteration not null");
  if (!radiosity_rho_ok(reflectivityScalar))
    return fail(c, VR_E_INVALID, "vr_debug_radiosity_time_iterations: the reflectivity must lie in [0, 1]");
  VR_TRY(radiosity_table_refusal(c, api));
  VR_HIP(c, hipSetDevice(c->device));
  RadiosityArgs a;
  VR_TRY(solve_begin(c, api, nullptr, reflectivityScalar, 0.f, a));
  float *const e[2] = {c->dRadE0.p, c->dRadE1.p};
  a.residual = c->dRadWords.p + 1;
  a.prevResidual = nullptr; // every launch runs, converged or not: this is a measurement
  hipEvent_t e0 = nullptr, e1 = nullptr;
  VR_HIP(c, hipEventCreate(&e0));
  hipError_t err = hipEventCreate(&e1);
  if (err == hipSuccess)
    err = hipMemsetAsync(a.residual, 0, 4, c->stream);
  if (err == hipSuccess)
    err = hipEventRecord(e0, c->stream);
  for (uint32_t k = 0; k < count && err == hipSuccess; ++k) {
    a.eIn = e[k & 1u];
    a.eOut = e[(k + 1u) & 1u];
    err = launch_radiosity_iterate(a, nontemporal != 0, c->stream);
  }
  if (err == hipSuccess)
    err = hipEventRecord(e1, c->stream);
  if (err == hipSuccess)
    err = hipEventSynchronize(e1);
  float ms = 0.f;
  if (err == hipSuccess)
    err = hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0);
  if (e1)
    (void)hipEventDestroy(e1);
  VR_HIP(c, err);
  *msPerIteration = ms / (float)count;
  return VR_OK;
}

int vr_radiosity_free_links(vr_context *c) {
  if (!c)
    return VR_E_INVALID;
  VR_HIP(c, hipSetDevice(c->device));
  VR_TRY(host_waits(c));
  c->radValid = false;
  c->dRadLinks.release();
  c->dRadDirect.release();
  c->dRadOrigOfLeaf.release();
  return VR_OK;
}

} // extern "C"
