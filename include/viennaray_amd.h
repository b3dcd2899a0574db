/* viennaray_amd.h — C ABI of the MI355X-native flux ray-tracing core.
 *
 * This is the drop-in boundary for ONE path of ViennaTools/ViennaRay: the work
 * done by Trace<T,D>::apply() (reference: include/viennaray/rayTrace.hpp:15-180,
 * rayTraceDisk.hpp:19-57, rayTraceTriangle.hpp:19-61 and the ray loop in
 * rayTraceKernel.hpp:32-426).  The reference has no FFI (header-only C++
 * templates); the entry points below are what a `viennaray::TraceDisk` /
 * `TraceTriangle` facade binds to (the headers under include/viennaray_amd/ are that facade,
 * INTEGRATION.md shows the binding).  Everything is `extern "C"`, plain pointers
 * and sizes; the library owns all HIP state.  NumericType on the device is
 * float (Embree is float internally: rayUtil.hpp:96-97).
 *
 * Ownership: every host pointer is read during the call and never retained
 * (the reference copies geometry into Embree buffers: rayGeometryDisk.hpp:123-176).
 * Status: every function returning int returns VR_OK (0) or a negative VR_E_*;
 * vr_last_error() gives the message.  HIP failures never abort the process.
 * Threading: one context per host thread (the reference's Trace objects are not
 * thread-safe either); a context binds one HIP device.
 */
#ifndef VIENNARAY_AMD_H
#define VIENNARAY_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vr_context vr_context;

enum {
  VR_OK = 0,
  VR_E_INVALID = -1,  /* bad argument / missing geometry or particle      */
  VR_E_HIP = -2,      /* HIP runtime error (no device, OOM, launch failure) */
  VR_E_STATE = -3     /* call order (e.g. get_flux before apply)           */
};

/* rayBoundary.hpp:10-14 */
enum { VR_REFLECTIVE_BOUNDARY = 0, VR_PERIODIC_BOUNDARY = 1, VR_IGNORE_BOUNDARY = 2 };
/* rayUtil.hpp:40-47 */
enum { VR_POS_X = 0, VR_NEG_X = 1, VR_POS_Y = 2, VR_NEG_Y = 3, VR_POS_Z = 4, VR_NEG_Z = 5 };
/* rayUtil.hpp:38 */
enum { VR_NORM_SOURCE = 0, VR_NORM_MAX = 1 };
/* vr_get_flux_device: no normalisation, the raw flux */
enum { VR_NORM_NONE = -1 };
/* particle kinds of the device registry (viennaray_amd/csrc/vr_particles.hpp):
 * 0, 1     the reference's built-ins DiffuseParticle / SpecularParticle (rayParticle.hpp:126-204)
 * 2        CONED_COSINE: surfaceReflection = ReflectionConedCosine(coneAngle) (rayReflection.hpp:52-120),
 *          collision like SpecularParticle
 * 3        DIFFUSE_COSINE: a DiffuseParticle with TWO data labels: label 0 += w, label 1 += w * max(0, -d.n)
 * 4        COVERAGE_STICKING: a DiffuseParticle whose sticking falls with the coverage of the primitive it meets:
 *          sticking * (1 - globalData.vector(params[0])[primID]) — reads Trace::setGlobalData (vr_set_global_data)
 * A model is a struct of __device__ functions {sticking, reflect, collide} appended to the registry's type list;
 * its position is its id, its parameters travel in vr_particle::params. */
enum { VR_PARTICLE_DIFFUSE = 0, VR_PARTICLE_SPECULAR = 1, VR_PARTICLE_CONED_COSINE = 2, VR_PARTICLE_DIFFUSE_COSINE = 3,
       VR_PARTICLE_COVERAGE_STICKING = 4 };
/* geometry kinds (rayGeometry.hpp:9) */
enum { VR_GEOMETRY_DISK = 0, VR_GEOMETRY_TRIANGLE = 1 };

/* rayUtil.hpp:65-76 (+ raysTerminated, a local of TraceKernel::apply) */
typedef struct vr_trace_info {
  uint64_t numRays;
  uint64_t totalRaysTraced;
  uint64_t nonGeometryHits;
  uint64_t geometryHits;
  uint64_t particleHits;
  uint64_t boundaryHits;
  uint64_t reflections;
  uint64_t raysTerminated;
  double time;          /* seconds: BVH build + ray loop, like the reference (Q10) */
  double timeBuild;     /* seconds: BVH build part of `time`                       */
  double timeTrace;     /* seconds: device pipeline gen+sort+trace (HIP events)     */
  double timeTraceKernel; /* seconds: the trace kernel(s) alone (HIP events)        */
  int32_t warning;
  int32_t error;
  uint64_t rngFullStates; /* diagnostic: rays that drew more than 156 numbers and continued
                             on the full 312-word engine state       */
  double timeGenKernel;   /* seconds: the ray generator kernel(s) alone (HIP events)  */
  uint32_t bvhRefits;     /* diagnostic: 1 if the resident BVH failed its first consistency check and was
                             re-fitted with agent-scope fences (expected 0; non-zero is a finding, not a
                             state to live with: the tests and smoke() assert 0)               */
  uint32_t bvhBuilds;     /* scene builds this context has run so far (a re-apply on unchanged geometry adds none) */
} vr_trace_info;

/* gpu::Particle-style POD (rayParticle.hpp:208-218): a built-in particle.
 * DIFFUSE ignores sourcePower (rayParticle.hpp:158 returns 1).             */
typedef struct vr_particle {
  int32_t kind;            /* VR_PARTICLE_*                                   */
  float sticking;          /* stickingProbability_                            */
  float sourcePower;       /* cosine exponent n of the source (SPECULAR only) */
  int32_t numMaterialSticking;      /* 0 = none                               */
  const int32_t *materialIds;       /* [numMaterialSticking] material id ...  */
  const float *materialSticking;    /* ... -> sticking override               */
  float coneAngle;                  /* CONED_COSINE: maxConeAngle in radians  */
  float meanFreePath;               /* getMeanFreePath(); <= 0: no scattering (rayParticle.hpp:113) */
  float params[8];                  /* the model's own parameters (registry models beyond the built-ins)      */
} vr_particle;

/* ---- life cycle (Trace::Trace / ~Trace, rayTrace.hpp:17-29) ------------- */
int vr_create(vr_context **out, int device);
void vr_destroy(vr_context *ctx);
const char *vr_last_error(const vr_context *ctx);
/* static: 1 if a HIP device is usable, 0 otherwise (never throws)           */
int vr_device_available(void);
const char *vr_version(void);

/* ---- geometry ------------------------------------------------------------
 * TraceDisk::setGeometry(points, normals, gridDelta[, diskRadius])
 * (rayTraceDisk.hpp:62-92).  points/normals: n x 3 floats (for D==2 the z
 * column is ignored, rayGeometryDisk.hpp:148-176).  diskRadius <= 0 selects
 * gridDelta * DiskFactor<D> (rayUtil.hpp:99-101).                           */
int vr_set_disks(vr_context *ctx, const float *points, const float *normals,
                 uint32_t n, float gridDelta, float diskRadius, int D);
/* vr_set_disks for a surface that already lives on the device (an advection step written in torch or HIP).
 * points / normals: DEVICE pointers on ctx's device, float32, row-major, `ld` floats per row (2 or 3; 2 only when
 * D == 2; with D == 2 and ld == 3 the third column is ignored, as vr_set_disks ignores it).  `stream`: the hipStream_t
 * the caller produced them on (NULL = the null stream); the library's stream waits for it by an event.  On return the
 * library has taken its own copy: the caller may overwrite or free its buffers at once.  Same argument checks and
 * effects as vr_set_disks; additionally refuses ld outside {2, 3} and pointers that are not device memory of ctx's
 * device (host, pinned and managed memory included).  A refusal leaves the previous geometry in place.  What comes
 * back to the host is the bounding box (six floats); the host copies of the rows are made only if a host path
 * (VR_HOST_BUILD, VR_HOST_SMOOTH, a smoothing overflow) asks for them.                                   */
int vr_set_disks_device(vr_context *ctx, const float *points, const float *normals, uint32_t n, uint32_t ld,
                        float gridDelta, float diskRadius, int D, void *stream);
/* TraceTriangle::setGeometry(TriangleMesh) (rayTraceTriangle.hpp:71-74;
 * normals per rayMesh.hpp:99-112).  verts: nverts x 3, tris: ntris x 3.      */
int vr_set_triangles(vr_context *ctx, const float *verts, uint32_t nverts,
                     const uint32_t *tris, uint32_t ntris, float gridDelta, int D);
/* vr_set_triangles for a mesh that already lives on the device (a meshing or advection step written in torch or HIP).
 * verts: DEVICE pointer on ctx's device to nverts rows of 3 float32; tris: DEVICE pointer to ntris rows of 3 uint32;
 * both produced on `stream` (the caller's hipStream_t, NULL = the null stream), which the library's stream waits for by
 * an event.  Same effects as vr_set_triangles (ntris < 2^27; here also nverts < 2^31); additionally refuses pointers
 * that are not device memory of ctx's device (host, pinned and managed memory included).  The indices are checked on the
 * device before anything else happens: an index >= nverts is refused with vr_set_triangles' message and the lowest
 * offending triangle.  Every refusal leaves the previous geometry in place and the context usable.  Accepted, one kernel
 * copies both buffers and makes the unit normals and areas, bit for bit those of vr_set_triangles; `stream` is made to
 * wait for it, so the caller may reuse its buffers with work queued on `stream` at once (from the host, or to free them,
 * after synchronising `stream`).  One synchronisation with the host per call:
 * seven words come back (the bounding box over all vertices and the index check).  The host copies are made only if a
 * host path (VR_HOST_BUILD) asks for them.  Non-finite vertices are the caller's error, as for vr_set_triangles. */
int vr_set_triangles_device(vr_context *ctx, const float *verts, uint32_t nverts, const uint32_t *tris, uint32_t ntris,
                            float gridDelta, int D, void *stream);
/* setMaterialIds (rayGeometry.hpp:17-24)                                    */
int vr_set_material_ids(vr_context *ctx, const int32_t *ids, uint32_t n);
/* vr_set_material_ids for ids that live on the device: ids is a DEVICE pointer on ctx's device to n int32 in the
 * caller's primitive order, produced on `stream` (NULL = the null stream).  A primitive beyond n has id 0; a geometry
 * with another primitive count resets the ids to 0.  One device-to-device copy, ordered by events on both sides as in
 * vr_set_global_data_device; the per-primitive sticking of a material-dependent particle and a stateful model's
 * material ids are then made on the device.  A refusal (not device memory of ctx's device) leaves the previous ids. */
int vr_set_material_ids_device(vr_context *ctx, const int32_t *ids, uint32_t n, void *stream);

/* ---- configuration (rayTrace.hpp:41-121) -------------------------------- */
int vr_set_boundary_conditions(vr_context *ctx, const int32_t *bcs, int n /* = D */);
int vr_set_source_direction(vr_context *ctx, int traceDirection);
int vr_set_primary_direction(vr_context *ctx, const float *dir3 /* NULL = off */);
int vr_set_particle(vr_context *ctx, const vr_particle *particle);
/* Several particles in ONE apply(), as the reference's gpu::Trace does (gpu/raygTrace.hpp:163-248: one launch per
 * particle, all with the seed of that apply): particle i's data labels follow particle i-1's in
 * vr_get_flux_data / vr_num_data; particles with the same source distribution share one generator pass (the rays
 * of ray index idx are the same for them).  runNumber advances once.                                         */
int vr_set_particles(vr_context *ctx, const vr_particle *particles, uint32_t n);
/* OPEN registration (the reference's GPU path registers user callables per particle at run time,
 * gpu/raygCallableConfig.hpp:7-18, gpu/raygTrace.hpp:163-248): `source` is HIP source text defining
 *     struct VrUserModel { static constexpr int kNumData; static constexpr bool kNeedsFull;
 *                          __device__ static float sticking(const ModelCtx &, unsigned primID, float base);
 *                          template <int D> __device__ static V3 reflect(const ModelCtx &, const V3 &rayDir, const V3 &n, Rng &, unsigned &);
 *                          template <class Credit> __device__ static void collide(const ModelCtx &, float w, const V3 &rayDir,
 *                                                                               const V3 &n, unsigned primID, Credit &&credit); };
 * (usually derived from a built-in model of viennaray_amd/csrc/vr_particles.hpp, overriding one member).  The library
 * compiles the extended trace kernels around it for gfx950 (hipcc --genco, cached by content under VR_CACHE_DIR or
 * /tmp) and loads the code object; *kind (>= VR_PARTICLE_USER_BASE) is then a valid vr_particle::kind of this context.
 * numData = VrUserModel::kNumData (1..4); flags: VR_MODEL_NEEDS_FULL = VrUserModel::kNeedsFull (the model is to be
 * combined with WDIST crediting / mean-free-path scattering, or brings heavy code of its own).  Needs hipcc at run time. */
enum { VR_PARTICLE_USER_BASE = 1000, VR_MODEL_NEEDS_FULL = 1 };
int vr_register_particle_model(vr_context *ctx, const char *name, const char *source, int numData, int flags, int32_t *kind);
/* ... a model with per-ray STATE (the reference's particle members / initNew, rayParticle.hpp:21-81): numState =
 * VrUserModel::kStateWords (0 .. 4; 0 is vr_register_particle_model).  A stateful model (kStateWords > 0, kNeedsFull =
 * true; VR_MODEL_NEEDS_FULL is implied) provides instead of sticking / reflect / collide
 *     __device__ static void init(const ModelCtx &, RayState &s, Rng &, unsigned &t2);            // initNew, before the source sample
 *     template <int D> __device__ static Reflection surface_reflection(const ModelCtx &, RayState &s, float w, const V3 &rayDir,
 *         const V3 &n, unsigned primID, int materialId, float baseSticking, Rng &, unsigned &t2); // {sticking, new direction}
 *     template <class Credit> __device__ static void collide(const ModelCtx &, const RayState &s, float w, const V3 &rayDir,
 *         const V3 &n, unsigned primID, int materialId, Credit &&credit);                       // no engine draws
 * (viennaray_amd/csrc/vr_particles.hpp; materialId: vr_set_material_ids of the original primitive, 0 without).  Its rays
 * come from SourceRandom (plain or with a primary direction); SourceGrid and host sources are refused at apply time. */
int vr_register_particle_model_ex(vr_context *ctx, const char *name, const char *source, int numData, int numState, int flags,
                                  int32_t *kind);
/* Trace::setGlobalData (rayTrace.hpp:137-145; handed to every surfaceCollision / surfaceReflection,
 * rayParticle.hpp:21-81): vector `vecIdx` (indexed by primitive id) and the scalars of the caller's TracingData,
 * copied to HBM and readable by the device particle models.  data == NULL drops the vector and those behind it. */
int vr_set_global_data(vr_context *ctx, uint32_t vecIdx, const float *data, uint32_t n);
int vr_set_global_scalars(vr_context *ctx, const float *data, uint32_t n);
/* vr_set_global_data for a vector that already lives on the device (coverages computed from the flux tensor).  data: a
 * DEVICE pointer on ctx's device, n floats; `stream`: the hipStream_t it was produced on (NULL = the null stream).  Same
 * semantics as vr_set_global_data (at most 16 vectors, any length, 0 beyond its length, data == NULL or n == 0 drops the
 * vector and those behind it); host-set and device-set vectors may be mixed on one context in any order.  The library's
 * stream waits for `stream` by an event, a kernel copies the vector into place, and `stream` waits for that copy: the
 * caller may overwrite its buffer with work queued on `stream` afterwards.  No host synchronisation unless the resident
 * rows have to move (a vector longer than any before, more vectors than before).  Refuses pointers that are not device
 * memory of ctx's device; a refusal leaves the vectors as they were.                                           */
int vr_set_global_data_device(vr_context *ctx, uint32_t vecIdx, const float *data, uint32_t n, void *stream);
/* VIENNARAY_USE_WDIST (CMakeLists.txt:15, rayTraceKernel.hpp:258-296) as a run-time switch: a hit's
 * weight is shared among the credited disks by inverse impact distance                       */
int vr_set_use_wdist(vr_context *ctx, int on);
/* setSource(SourceGrid) (raySourceGrid.hpp): explicit origins, direction from the particle's cosine
 * power; numRays = n * numRaysPerPoint.  n == 0 = resetSource() (rayTrace.hpp:53-61)            */
int vr_set_source_grid(vr_context *ctx, const float *points3, uint32_t n);
/* setSource(any other Source) (raySource.hpp:10-19): the facade runs the callback on the host and
 * hands over ray idx -> origin, direction, engine outputs consumed.  n == 0 = resetSource()      */
int vr_set_host_rays(vr_context *ctx, const float *org3, const float *dir3, const uint32_t *draws, uint64_t n);
/* Source::getInitialRayWeight(idx) (raySource.hpp:18; rayTraceKernel.hpp:124,316-328,435-460) of the rays given
 * with vr_set_host_rays: start weight of ray idx and scale of the roulette's thresholds.  n == 0: all 1          */
int vr_set_host_ray_weights(vr_context *ctx, const float *weights, uint64_t n);
/* Source::getSourceArea() (raySource.hpp:17) for normalizeFlux(SOURCE) (rayTraceDisk.hpp:127,
 * rayTraceTriangle.hpp:113); area <= 0: SourceRandom's (raySourceRandom.hpp:40-47, the bbox source face)       */
int vr_set_source_area(vr_context *ctx, float area);
/* A user Source (raySource.hpp:10-19: getOriginAndDirection(idx, rng), getInitialRayWeight(idx)) as DEVICE code, sampled in
 * the ray generator instead of on the host.  `source` is HIP text that defines
 *     struct VrUserSource {
 *       static constexpr bool kHasWeight = false;  // true: `weight` is the ray's start weight (getInitialRayWeight)
 *       template <int D, class Draw>
 *       __device__ static void sample(const SourceCtx &s, unsigned long long idx, Draw &&draw, V3 &org, V3 &dir, float &weight);
 *     };
 * draw() returns the next raw 64-bit output of ray idx's engine — any number of calls, different from ray to ray;
 * canon_f32(draw()) / canon_f64(draw()) are the reference's uniform float / double.  `dir` is used as returned: the model
 * normalises it (vnormalize), as the reference's callback does.  SourceCtx (viennaray_amd/csrc/vr_types.hpp): the adjusted
 * bounding box, the source plane, rayDir / firstDir / secondDir / posNeg, gridDelta, the particle's source power,
 * params[16] and one float table in device memory (table, tableCount).  The library compiles the ray generator around the
 * text for gfx950 (hipcc --genco, cached by content like a particle model's; no trace kernel is compiled) and loads it;
 * *sourceId is then valid for vr_set_source_model on this context.  flags: VR_SOURCE_HAS_WEIGHT exactly when kHasWeight is
 * true.  A text that does not compile returns VR_E_INVALID with the compiler's error lines in vr_last_error; the context
 * stays usable.  Needs hipcc at run time.                                                                            */
enum { VR_SOURCE_HAS_WEIGHT = 1 };
int vr_register_source_model(vr_context *ctx, const char *name, const char *source, int flags, int32_t *sourceId);
/* The source of the next applies is model `sourceId` (< 0: back to SourceRandom) with params[0 .. nparams) (nparams <= 16,
 * zeros behind them) and a table of ntable floats, copied to the device here (NULL / 0: none).  numRays == 0: the ray
 * count is SourceRandom's (numRaysFixed, or numRaysPerPoint per primitive); > 0: the source's own (<= 2^32 - 1, as for
 * host rays).  It replaces and is replaced by a source grid, host rays and a surface source; vr_set_source_area keeps
 * supplying getSourceArea().  Without kHasWeight every ray starts with weight 1 and an absorbing particle keeps its
 * absorbing kernel, as under weightless host rays.  vr_set_ray_range and vr_apply_sharded work unchanged: the sample
 * depends on the global ray index only.  A stateful particle model cannot be combined with it (refused at prepare).
 * A refused call leaves the source in force as it was.                                                              */
int vr_set_source_model(vr_context *ctx, int32_t sourceId, const float *params, uint32_t nparams, const float *table,
                        uint32_t ntable, uint64_t numRays);
/* ... its table from DEVICE memory of the context's device (ntable == 0: no table): copied on the context's stream behind
 * what `stream` (NULL: the null stream) holds now, and `stream` then waits for the copy — the contract of
 * vr_set_global_data_device: the caller may reuse dTable in the order of its stream; nothing waits on the host unless the
 * library's buffer has to grow.  Refused (no source model in force, not device memory of this device): the previous
 * table stays.                                                                                                      */
int vr_set_source_model_table_device(vr_context *ctx, const float *dTable, uint32_t ntable, void *stream);
/* setSurfaceSource / clearSurfaceSource (gpu/raygTrace.hpp:267-297; sample: gpu/raygSource.hpp:13-26, 65-81, 105-118):
 * the rays start ON the n given points — numRaysFixed if set, else numRaysPerPoint, rays per point (:134-149), global ray
 * idx at point idx / raysPerPoint — from positions3[3 j] + unit normal * sourceOffset, along a power-1 cosine
 * distribution about normals3[3 j] (any non-zero length), with start weight weights[j] (finite, >= 0), sampled on the
 * device.  normalizeFlux(SOURCE) uses sourceArea (> 0) while it is set (gpu/raygTraceDisk.hpp:90-91,
 * gpu/raygTraceTriangle.hpp:45-46).  The tables are copied to the device by this call.  Replaces a source grid and host
 * rays, and is replaced by them; n == 0 = clearSurfaceSource().  An invalid argument leaves the previous source set.   */
int vr_set_surface_source(vr_context *ctx, const float *positions3, const float *normals3, const float *weights, uint32_t n,
                          float sourceArea, float sourceOffset);
/* vr_set_surface_source for tables that live on the device (the surface the tracer already holds, weights computed from
 * the first pass's flux tensor).  positions / normals: DEVICE pointers on ctx's device to n rows of `ld` floats (2 or 3;
 * 2 only on a 2-D geometry, the third column then reads 0), weights: n floats, all produced on `stream` (NULL = the null
 * stream).  sourceArea / sourceOffset are checked on the host; the rows are checked on the device by the kernel that
 * packs them — position finite, normal of positive finite length, weight finite and >= 0 — and ONE word comes back: a
 * refusal names the row and the check that vr_set_surface_source would have named, in the same words, and leaves the
 * previous source in place.  On return the library holds its own copy.  n == 0 = clearSurfaceSource().              */
int vr_set_surface_source_device(vr_context *ctx, const float *positions, const float *normals, const float *weights,
                                 uint32_t n, uint32_t ld, float sourceArea, float sourceOffset, void *stream);
int vr_set_number_of_rays_per_point(vr_context *ctx, uint64_t n);
int vr_set_number_of_rays_fixed(vr_context *ctx, uint64_t n);
int vr_set_max_reflections(vr_context *ctx, uint32_t n);
int vr_set_max_boundary_hits(vr_context *ctx, uint32_t n);
int vr_set_rng_seed(vr_context *ctx, uint32_t seed);
int vr_set_use_random_seeds(vr_context *ctx, int useRandom);
/* KernelConfig::runNumber (rayUtil.hpp:93); apply() increments it           */
int vr_set_run_number(vr_context *ctx, uint32_t runNumber);
int vr_get_run_number(const vr_context *ctx, uint32_t *runNumber);

/* Multi-GPU sharding hook (not in the reference): trace only the global ray
 * indices [first, first+count).  count == 0 restores "all rays".  Ray idx
 * stays global, so the union over ranks reproduces the single-device stream
 * (rayTraceKernel.hpp:118-121).                                             */
int vr_set_ray_range(vr_context *ctx, uint64_t first, uint64_t count);
/* Number of ranks whose flux accumulators the caller is going to SUM (default 1; vr_apply_sharded sets it by itself).
 * The accumulators are int64 fixed point (weight * 2^VR_FLUX_FRAC_BITS): one primitive and data label holds
 * 2^23 = 8.39e6 weight units per apply(), divided by `world` rounded up to a power of two so that the signed sum over
 * the ranks cannot wrap either.  Beyond that vr_apply_finish / vr_apply FAILS (VR_E_STATE, TraceInfo.error = 1,
 * "flux accumulator overflow") instead of returning wrapped flux — the reference's float sums (rayTraceKernel.hpp:
 * 348-360, rayParticle.hpp:148-156) stall near 2^24 at that point.                                                  */
int vr_set_world_size(vr_context *ctx, uint32_t world);

/* Not in the reference (its ray loop allocates nothing per apply): apply() once per time step with a ray
 * count that follows the moving surface re-sizes the HBM ray stream; reserve it for the largest count
 * expected.  (Without a reservation the stream grows by half again when it must, and is kept.)             */
int vr_reserve_rays(vr_context *ctx, uint64_t n);

/* ---- run (Trace::apply) -------------------------------------------------- */
int vr_apply(vr_context *ctx);
/* Same, split for benchmarking: build = bbox/boundary/areas/BVH/uploads,
 * launch = zero accumulators + enqueue the trace kernel on the context's
 * stream (asynchronous), finish = wait + read counters.                     */
int vr_apply_prepare(vr_context *ctx);
int vr_apply_launch(vr_context *ctx);
int vr_apply_finish(vr_context *ctx);

/* Multi-GPU apply() (the reference has no distributed layer): one process per GPU,
 * geometry and BVH replicated, rank r traces the r-th contiguous share of the global ray indices
 * (ray idx keeps its global value, so the union reproduces the single-device stream,
 * rayTraceKernel.hpp:118-121), and the per-primitive int64 accumulators plus the seven counters
 * are summed over the ranks by `reduce` — an in-place sum all-reduce of `count` int64 in DEVICE
 * memory enqueued on `hipStream` (0 = ok).  vr_rccl_allreduce (viennaray_amd_rccl.h) is that
 * callback on RCCL over xGMI.  Afterwards every rank holds the full result of Trace::apply().   */
typedef int (*vr_allreduce_fn)(void *user, void *devInt64, size_t count, void *hipStream);
int vr_apply_sharded(vr_context *ctx, int rank, int world, vr_allreduce_fn reduce, void *user);

/* ---- results ------------------------------------------------------------- */
uint32_t vr_num_primitives(const vr_context *ctx);
/* getLocalData().getVectorData(0) (rayTrace.hpp:135): raw, un-normalised     */
int vr_get_flux(vr_context *ctx, float *out, uint32_t n);
int vr_get_flux_f64(vr_context *ctx, double *out, uint32_t n);
/* getLocalData().getVectorData(dataIdx) for particles with several data labels
 * (AbstractParticle::getLocalDataLabels, rayParticle.hpp:75-78; rayTraceDisk.hpp:40-47)      */
uint32_t vr_num_data(const vr_context *ctx);
int vr_get_flux_data(vr_context *ctx, uint32_t dataIdx, float *out, uint32_t n);
int vr_get_trace_info(const vr_context *ctx, vr_trace_info *out);
/* the counters of particle `particleIdx` of a multi-particle apply (vr_get_trace_info holds their sums)   */
int vr_get_particle_trace_info(const vr_context *ctx, uint32_t particleIdx, vr_trace_info *out);
/* which trace_kernel variant the last vr_apply_prepare selected: 0 general (reflection, roulette,
 * RNG), 1 absorbing + flat scene, 2 absorbing + structured scene, 3 general + flat scene,
 * 4 general, scene of a few hundred primitives resident in LDS             */
int vr_get_trace_mode(const vr_context *ctx, int32_t *mode);
/* normalizeFlux / smoothFlux (rayTraceDisk.hpp:103-193, rayTraceTriangle.hpp:92-136), in place on
 * a caller buffer; both run as HIP kernels on the resident areas / neighbourhood (upload, kernel,
 * download)                                                                                   */
int vr_normalize_flux(vr_context *ctx, float *flux, uint32_t n, int normType);
/* getLocalData().getVectorData(0) + normalizeFlux fused on the device: the raw flux never visits
 * the host (accumulators -> float -> flux * sourceArea / (numRays * area), one download)     */
int vr_get_flux_normalized(vr_context *ctx, float *out, uint32_t n, int normType);
int vr_smooth_flux(vr_context *ctx, float *flux, uint32_t n, int numNeighbors);
/* The flux of data label `dataIdx` in the CALLER's primitive order, float32, written to DEVICE memory `out`
 * (n = numPrims, on ctx's device): accumulators -> float -> normalizeFlux(normType; VR_NORM_NONE = raw) ->
 * smoothFlux(numNeighbors; 0 = none), bit for bit what vr_get_flux_data, vr_normalize_flux and vr_smooth_flux return
 * one after the other.  The work is enqueued on the context's stream behind what `stream` (the caller's, NULL = the
 * null stream) holds at the call, and `stream` is made to wait for it by an event: without smoothing there is no host
 * synchronisation and no host copy.  With smoothing one word is read back (the kernels' overflow flag); if it is set
 * the host smoothing runs and its result is uploaded.                                                     */
int vr_get_flux_device(vr_context *ctx, uint32_t dataIdx, float *out, uint32_t n, int normType, int numNeighbors,
                       void *stream);
/* ---- per-primitive values at the caller's points (not in the reference) ------------------------------------------------
 * One float per primitive of the geometry in force — a flux, a coverage, anything — is mapped to m query points that
 * need not be primitives: grid points, the next surface's points, a coarser or finer point set.  The definition:
 *   f[j]   one float per primitive, in the caller's primitive order;  p_i: the m query points;  m_i: optional query
 *          normals of any non-zero length, normalised in the kernel;  R >= 0: a radius.
 *   c_j    the centre of primitive j: a disk's is the caller's point; a triangle's is its centroid
 *          ((v0 + v1) + v2) * (1.f / 3.f), taken per component in float32.
 *   D == 2 the z components of p_i, c_j and of the normals are ignored (2-D triangle strips included).
 *   d_ij = |p_i - c_j|, plain Euclidean: the side walls' periodicity is NOT applied.  Primitive j is in range iff d_ij < R.
 *   w_ij = (1 - d_ij / R) * g_ij;  g_ij = 1 without query normals, else max(0, n_j . m^_i), n_j the unit normal the
 *          library holds for the primitive.
 *   out[i] = sum_j w_ij f[j] / sum_j w_ij over the primitives in range, if sum_j w_ij > 0;
 *          = f[j*] otherwise, j* the primitive whose centre is nearest to p_i, the lowest original id on an exact tie;
 *            normals play no part in this fallback.  It covers R == 0, nothing in range and every in-range normal
 *            facing away.
 *   A query point with a coordinate that is not finite gives out[i] = NaN; the call still returns VR_OK.
 *   m == 0 is VR_OK and touches nothing.
 * Two calls with the same inputs on the same built scene give the same bits.  Another build of the same geometry (a
 * geometry set anew) may differ in the last bits: the sums run in the order of the walk over the resident BVH.
 * Refused, `out` untouched and the context usable, message in vr_last_error:
 *   VR_E_INVALID  n != vr_num_primitives, ld outside {2, 3}, ld == 2 with D == 3, a radius that is negative or not
 *                 finite, a null pointer where one is needed; a pointer that is not device memory of ctx's device;
 *   VR_E_STATE    no scene build is resident for the geometry in force: nothing has been prepared yet (vr_apply or
 *                 vr_apply_prepare builds it), or the geometry was set since.  vr_get_flux_at_points_device: whatever
 *                 vr_get_flux_device refuses as well.
 * Streams: as vr_get_flux_device — enqueued on the context's stream behind what `stream` holds at the call, `stream`
 * made to wait for the result by an event; no host synchronisation unless a work buffer of the library has to grow
 * (the first call, a larger m), or, with smoothing, for vr_get_flux_device's one word.
 *
 * values: DEVICE, n = vr_num_primitives floats, caller's order; points / normals: DEVICE, m rows of ld (2 or 3; 2 only with D == 2)
 * floats, normals may be NULL; out: DEVICE, m floats; stream rules of vr_get_flux_device */
int vr_map_to_points_device(vr_context *ctx, const float *values, uint32_t n, const float *points, const float *normals,
                            uint32_t m, uint32_t ld, float radius, float *out, void *stream);
/* the same from and to host arrays (m x 3): upload, kernel, download */
int vr_map_to_points(vr_context *ctx, const float *values, uint32_t n, const float *points3, const float *normals3,
                     uint32_t m, float radius, float *out);
/* vr_get_flux_device(dataIdx, normType, numNeighbors) into a work buffer, then the map: the flux never leaves the device */
int vr_get_flux_at_points_device(vr_context *ctx, uint32_t dataIdx, int normType, int numNeighbors, const float *points,
                                 const float *normals, uint32_t m, uint32_t ld, float radius, float *out, void *stream);
/* ---- closest-hit queries for the caller's rays (not in the reference) ---------------------------------------------------
 * "Where does this ray hit?" for m rays of the caller against the resident scene: the BVH, the packed primitives and
 * the side walls with their REFLECTIVE / PERIODIC / IGNORE rules, exactly as an apply() traces them.  The definition:
 *   A ray is an origin and a direction.  The direction is used as the tracer uses a host ray's (vr_set_host_rays): as it
 *     stands, NOT normalised — except on a 2-D scene, where a direction with z != 0 has its z dropped and is then
 *     normalised (rows of 2 floats have z = 0).  So t, and with it dist and tmax, runs in units of the direction's
 *     length wherever the direction is used as it stands.
 *   A segment: the closest hit of the ray from its origin among the primitives and the eight wall triangles, from
 *     parameter tnear on; ties go to the smaller t, then to a wall, then to the lower original primitive id (the
 *     tracer's rule).  The first segment uses the caller's tnear (pass 1e-4f for the tracer's), every later one 1e-4f.
 *   A geometry hit ends the ray.  A miss ends the ray.  A wall hit ends the ray unless VR_CAST_FOLLOW_BOUNDARIES is
 *     set; with it the ray goes on from the wall as the tracer's would — reflected, wrapped to the opposite wall, or
 *     passed through from its back side — unless the wall is IGNORE (the ray leaves: a miss) or this wall is one more
 *     than vr_set_max_boundary_hits allows (the ray stops on it).
 *   dist  the float32 sum of the segments' t, added in segment order.
 *   tmax >= 0 (INFINITY: none): the result is that of the unbounded cast with every outcome whose dist > tmax turned
 *     into a miss.  A hit at exactly tmax counts.
 * Outputs, one row per ray, in the caller's order:
 *   prim[i]   >= 0: the original id of the primitive hit (what vr_debug_intersect calls primID);
 *             VR_CAST_MISS: nothing — the ray left the scene, passed an IGNORE wall, or dist exceeds tmax;
 *             VR_CAST_WALL: the ray stopped on a wall (following is off, or the boundary-hit budget ran out).
 *   dist[i]   as above; +INFINITY for VR_CAST_MISS.
 *   hitPoints[3 i ..]  (optional) origin + direction * t of the LAST segment, the tracer's own expression, where the ray
 *             ended on a primitive or a wall; NaN for VR_CAST_MISS.
 *   boundaryHits[i]  (optional) the walls the ray was continued at.  With a finite tmax a VR_CAST_MISS reports 0 (such a
 *             ray may have been stopped before its end); without one it reports the walls passed before the ray left.
 * Same bits whatever the order the rays are walked in (VR_CAST_SORT_MIN: from that many rays on they are walked in
 * the Morton order of their origins), and however a set of rays is split over calls.
 * Refused, the outputs untouched and the context usable, message in vr_last_error:
 *   VR_E_INVALID  a null origins / directions / prim / dist with m > 0; ld outside {2, 3}, ld == 2 with D == 3; tnear or
 *                 tmax negative or NaN; a flag bit other than VR_CAST_FOLLOW_BOUNDARIES; (device form) a pointer that is
 *                 not device memory of ctx's device;
 *   VR_E_STATE    nothing to cast against: no vr_apply / vr_apply_prepare yet, or the geometry, the boundary conditions,
 *                 the source direction (the walls and the BVH's child order follow them) or another setting that makes
 *                 the next prepare redo the scene's configuration changed since; or the scene was built by the host
 *                 builder (VR_HOST_BUILD).
 * The call reads what the last prepare left and changes nothing of it: it prepares nothing, a finished apply's result
 * stays, and a later apply gives the bits it would have given without the cast.  m == 0 is VR_OK after the argument
 * checks.  Streams: as vr_map_to_points_device — on the context's stream, so ordered with applies; `stream` waits for
 * the result by an event; no host synchronisation unless a work buffer has to grow.
 *
 * origins / directions: DEVICE, m rows of ld (2 or 3; 2 only with D == 2) floats; prim / dist: DEVICE, m words each;
 * hitPoints: NULL or DEVICE m x 3 floats; boundaryHits: NULL or DEVICE m words */
#define VR_CAST_FOLLOW_BOUNDARIES 1u
#define VR_CAST_MISS (-1)
#define VR_CAST_WALL (-2)
int vr_cast_rays_device(vr_context *ctx, const float *origins, const float *directions, uint32_t m, uint32_t ld,
                        float tnear, float tmax, uint32_t flags, int32_t *prim, float *dist, float *hitPoints,
                        uint32_t *boundaryHits, void *stream);
/* the same from and to host arrays (m x 3): upload, kernel, download */
int vr_cast_rays(vr_context *ctx, const float *origins3, const float *directions3, uint32_t m, float tnear, float tmax,
                 uint32_t flags, int32_t *prim, float *dist, float *hitPoints, uint32_t *boundaryHits);
/* ---- gather flux (not in the reference): per-primitive direct flux by rays cast FROM the surface -----------------------
 * From each primitive of a range, `samples` rays into its own hemisphere: what share of the source does it see?  Every
 * primitive gets the same number of samples whatever its depth; an unoccluded flat surface under a power-1 source comes
 * out as exactly 1.  With an emission table the same call is one radiosity (Neumann) iteration.  The definition:
 * Scene   the resident scene of the last vr_apply / vr_apply_prepare (VR_E_STATE as vr_cast_rays_device).  a = the tracing
 *         axis; u = the unit vector along a FROM the surface TO the source plane.  Primary direction, source kind and
 *         the particle list play no part.
 * Primitive i (original id)   origin o_i: the disk centre, or the triangle's centroid rebuilt from the tracer's packed
 *         record ((v0 + v1 + v2) / 3 with v1 = v0 - e1, v2 = v0 + e2).  Normal m_i: the stored disk normal, or the
 *         tracer's unit triangle normal, normalised once more.
 * Sample k = 64 c + j of primitive i   chunk c owns one std::mt19937_64 seeded with tea<3>(i, S + c), S = the context's rng
 *         seed (vr_set_rng_seed) XOR 0x47415448; sample j takes its outputs 2j and 2j + 1 as r1, r2 (libstdc++'s uniform
 *         float).  vr_set_use_random_seeds does not apply: the call is a pure function of scene, seed and arguments.
 *         Direction w, VR_GATHER_NORMAL: D = 3 the cosine law about m_i as the surface source builds it (cos = sqrtf(r2),
 *           azimuth 2 pi r1, Frisvad basis, normalised); D = 2 the in-plane cosine law, sin(phi) = 2 r1 - 1 about m_i, z = 0
 *           (r2 is drawn and unused).
 *         Direction w, VR_GATHER_SOURCE: a sample of the SOURCE's law about u, the tracer's own (cos(theta) = powf(r2,
 *           1 / (n + 1)), azimuth 2 pi r1, in the source frame; in 2-D z is dropped and the rest normalised).
 * Walk    as vr_cast_rays with VR_CAST_FOLLOW_BOUNDARIES and tnear 1e-4f from o_i along w: closest hit with the tracer's
 *         tie rule, walls followed up to vr_set_max_boundary_hits.  A geometry hit ENDS the sample: there is no
 *         pass-through of a disk's back face as in a forward apply (hitFromBack); it matters only at the open rims of
 *         disk clouds.
 * Weight  n = cosinePower, c = u . w of the INITIAL direction (the side walls are parallel to a: following them never
 *         changes c).  The walls span the box up to the source plane, so a sample that ends as a miss with c > 0 and
 *         passed no IGNORE wall has crossed the source rectangle:
 *           reached the source:  NORMAL  g_D(n) c^(n - 1), g_3 = (n + 1) / 2, g_2 = 2 / C_n, C_n = sqrt(pi) Gamma((n + 1) / 2)
 *                                        / Gamma(n / 2 + 1); for n == 1 exactly g = 1 and no power is taken
 *                                SOURCE  max(0, m_i . w) / c; a sample with m_i . w <= 0 weighs 0 and is not walked
 *           hit primitive j on its front side (direction at the hit . m_j < 0), emission given:  emission[j]
 *           everything else: 0 — a back-side hit, a miss with c <= 0, a sample that left through an IGNORE wall or was
 *           stopped on a wall by the budget, a front-side hit without a table.
 * Result  out[i - primFirst] = (float)((double)sum_k q(w_k) / 2^VR_FLUX_FRAC_BITS / samples), q(w) = (int64)(w * 2^
 *         VR_FLUX_FRAC_BITS + 0.5), the flux accumulators' quantisation.  A weight that is not positive (NaN
 *         included) counts 0; one above wmax = 2^22 / (samples rounded up to a power of two) counts wmax — 1024 at 4096
 *         samples — so that no sum can leave an int64 whatever the emission table holds: an emission above wmax is cut
 *         to it, and so is the rare SOURCE weight with c below m_i . w / wmax.  The sum is an exact int64 sum: the same bits for any launch shape, order, and any
 *         split of the primitive range over calls.  Units are SOURCE-normalised: an unoccluded primitive facing the
 *         source between walls that are not IGNORE is 1; emission is in the same units (incoming flux x reflectivity).
 * Variance per sample: NORMAL w <= g c^(n-1) <= g, so Var <= F (g - F); SOURCE second moment <= (n + 1) / (2 (n - 1)), and
 * <= 1 / (n - 1) for m_i normal to u — hence VR_GATHER_SOURCE needs n >= 2.
 * Refused, out untouched and the context usable, message in vr_last_error:
 *   VR_E_INVALID  samples == 0; primFirst + primCount > vr_num_primitives; cosinePower not finite or < 1; mode not 0 / 1;
 *                 g_D(cosinePower) > wmax of `samples` (a NORMAL weight, at most g, would be cut: samples x g beyond 2^22);
 *                 VR_GATHER_SOURCE with cosinePower < 2 or with an emission table; out null with primCount > 0; (device
 *                 form) a pointer that is not device memory of ctx's device.  primCount == 0 is VR_OK after the checks.
 *   VR_E_STATE    as vr_cast_rays_device.
 * Streams, work buffers and "changes nothing of a finished apply; the next apply gives the bits it would have given": as
 * vr_cast_rays_device.  The int64 sums live in a work buffer of the context that grows on demand.
 *
 * emission: NULL or DEVICE, vr_num_primitives floats by original id; out: DEVICE, primCount floats */
#define VR_GATHER_NORMAL 0u
#define VR_GATHER_SOURCE 1u
int vr_gather_flux_device(vr_context *ctx, uint32_t primFirst, uint32_t primCount, uint32_t samples, float cosinePower,
                          uint32_t mode, const float *emission, float *out, void *stream);
/* the same from and to host arrays: upload, kernels, download */
int vr_gather_flux(vr_context *ctx, uint32_t primFirst, uint32_t primCount, uint32_t samples, float cosinePower,
                   uint32_t mode, const float *emission, float *out);
/* o_i, m_i and the directions of samples first .. first + count - 1 of primitive `prim`, as the gather builds them (host
 * arrays: 3, 3 and count x 3 floats) */
int vr_debug_gather_samples(vr_context *ctx, uint32_t prim, uint32_t first, uint32_t count, uint32_t mode,
                            float cosinePower, float *origin3, float *normal3, float *directions3);
/* ---- path gather (not in the reference): multi-bounce flux by paths traced BACK from the surface ------------------------
 * A mirror reflection is its own reverse and keeps etendue: a sample cast from primitive i can be followed through its
 * reflections until it reaches the source plane, and then brings back the source's radiance in its FINAL direction times
 * the product of the reflectivities on the way — the multi-bounce incoming flux of a specularly reflected species with
 * sticking below 1, with the same number of samples at every depth.  With a cosine re-emission at each vertex the same
 * loop is the unbiased estimate of the diffuse steady state (vr_radiosity_solve's fixed point) without a link table.
 * Scene, range, o_i, m_i, sample numbering, chunk engines and the INITIAL direction are exactly those of vr_gather_flux
 * in VR_GATHER_NORMAL mode: sample k of primitive i starts along the same bits.  What differs:
 * Segment  as vr_gather_flux: a followed cast, tnear 1e-4f, walls by their boundary conditions.  The
 *          vr_set_max_boundary_hits budget is counted over the WHOLE path, as the tracer counts it over a ray's life; a
 *          reflection does not reset it.
 * Vertex   a front-side hit of primitive j (direction at the hit . n_j < 0, n_j the normal the tracer tests sides
 *          against: the stored disk normal, the tracer's unit triangle normal) with fewer than maxBounces bounces made:
 *          T <- T * rho[j] (one float32 multiply, from T = 1; rho by original id, or the scalar).  T == 0: the path ends
 *          with weight 0.  Otherwise it goes on from the hit point (origin + direction * t, the tracer's restart) along
 *            VR_GATHER_REFLECT_SPECULAR  the tracer's mirror direction 2 (n_j . -d) n_j + d of the unprojected direction d
 *                                        (operation order: f = 2 * ((n.x * -d.x + n.y * -d.y) + n.z * -d.z); f * n.x - -d.x,
 *                                        ...), in 2-D followed by the tracer's projection (z dropped, then normalised);
 *            VR_GATHER_REFLECT_DIFFUSE   the cosine law about n_j as vr_gather_flux builds it about m_i (D = 3: cos =
 *                                        sqrtf(r2), azimuth 2 pi r1, Frisvad basis, normalised; D = 2: sin(phi) = 2 r1 - 1),
 *                                        from two uniforms of a COUNTER draw: with tea<8> the eight-round form of the
 *                                        tracer's seed hash, key = tea<8>(i, (S ^ 0x50415448) + k) for the path's starting
 *                                        primitive i (original id), sample index k and the context's rng seed S;
 *                                        r1, r2 = (float)(tea<8>(key, 2 b + {0, 1}) >> 8) * 2^-24 at bounce b = 0, 1, ...
 *                                        A pure function of (seed, i, k, b): nothing of chunks, ranges or earlier samples.
 * Ends     the source plane reached — a miss that passed no IGNORE wall, with c_end = u . w_end > 0 of the FINAL
 *          direction: weight T g_D(n) c_end^(n - 1), vr_gather_flux's NORMAL rule on c_end, then one multiply by T.
 *          Everything else weighs 0: a back-side hit, an IGNORE wall, the boundary-hit budget spent, a front-side hit
 *          with maxBounces bounces made (VR_GATHER_END_BOUNCES), T == 0 (VR_GATHER_END_ABSORBED).
 * Result   q(), wmax(samples), the exact int64 sum and the final division of vr_gather_flux; weights are at most g, so the
 *          same samples x g <= 2^22 refusal applies.  The same bits for any split of the range over calls and any launch
 *          shape; a pure function of scene, vr_set_rng_seed, vr_set_max_boundary_hits and arguments.  With maxBounces == 0,
 *          or reflectivity 0 everywhere, the result has the bits of vr_gather_flux(primFirst, primCount, samples,
 *          cosinePower, VR_GATHER_NORMAL, NULL).  Units: the SOURCE-normalised INCOMING flux.
 * Variance per sample: w <= g, so Var <= F (g - F) as for the gather.  The estimate is truncated at maxBounces bounces: it
 *          lacks at most rho_max^(maxBounces + 1) g.
 * Refused, out untouched and the context usable, message in vr_last_error:
 *   VR_E_INVALID  what vr_gather_flux_device refuses in VR_GATHER_NORMAL mode; reflection not 0 / 1; maxBounces above
 *                 VR_GATHER_MAX_BOUNCES; a reflectivity that is NaN, negative or above 1 (a table is checked on the device,
 *                 ONE word back; the message names the lowest such index); (device form) a pointer that is not device
 *                 memory of ctx's device.  primCount == 0 is VR_OK after the checks.
 *   VR_E_STATE    as vr_gather_flux_device.
 * Streams, work buffers and "changes nothing of a finished apply": as vr_gather_flux_device; the host waits once for the
 * verdict on a reflectivity table.
 *
 * reflectivity: NULL (reflectivityScalar counts) or DEVICE, vr_num_primitives floats by original id; out: DEVICE,
 * primCount floats */
#define VR_GATHER_REFLECT_SPECULAR 0u
#define VR_GATHER_REFLECT_DIFFUSE 1u
#define VR_GATHER_MAX_BOUNCES 65535u
int vr_gather_paths_device(vr_context *ctx, uint32_t primFirst, uint32_t primCount, uint32_t samples, float cosinePower,
                           uint32_t reflection, uint32_t maxBounces, const float *reflectivity, float reflectivityScalar,
                           float *out, void *stream);
/* the same from and to host arrays: upload, kernels, download */
int vr_gather_paths(vr_context *ctx, uint32_t primFirst, uint32_t primCount, uint32_t samples, float cosinePower,
                    uint32_t reflection, uint32_t maxBounces, const float *reflectivity, float reflectivityScalar, float *out);
/* ONE path — sample `sample` of primitive `prim` — as the call above walks it, through the same device functions (host
 * arrays; reflectivity: NULL or vr_num_primitives HOST floats).  Vertex 0 is the starting primitive, every later vertex a
 * geometry hit.  vertexIds[v]: the original id; vertexData[12 v ..]: the point (o_i, then hit points), the arriving
 * direction (NaN for vertex 0), the normal used (m_i, then n_j) and the leaving direction (NaN where the path ends on the
 * vertex), three floats each, unprojected.  Up to maxVertices vertices are stored; *numVertices counts all of them.
 * *end: how the path ended (VR_GATHER_END_*); finalDirection3: the direction it went along last; *throughput: T;
 * *weight: the unquantised weight.  Any of the five outputs behind vertexData may be NULL.  Refused as vr_gather_paths
 * for (prim, 1 primitive, 1 sample); also sample >= 2^22 (no call has that many) and maxVertices above
 * VR_GATHER_MAX_BOUNCES + 2 */
#define VR_GATHER_PATH_VERTEX_FLOATS 12u
#define VR_GATHER_END_MISS 0     /* reached the source plane (weight 0 still if c_end <= 0) */
#define VR_GATHER_END_IGNORED 1  /* left through an IGNORE wall */
#define VR_GATHER_END_WALL 2     /* stopped on a wall: the boundary-hit budget is spent */
#define VR_GATHER_END_BACK 4     /* hit a primitive on its back side */
#define VR_GATHER_END_BOUNCES 5  /* a front-side hit with maxBounces bounces made */
#define VR_GATHER_END_ABSORBED 6 /* a front-side hit that took the throughput to 0 */
int vr_debug_gather_path(vr_context *ctx, uint32_t prim, uint32_t sample, float cosinePower, uint32_t reflection,
                         uint32_t maxBounces, const float *reflectivity, float reflectivityScalar, uint32_t maxVertices,
                         uint32_t *vertexIds, float *vertexData, uint32_t *numVertices, uint32_t *end,
                         float *finalDirection3, float *throughput, float *weight);
/* ---- gather to a target error (not in the reference): per-primitive sums, standard error, adaptive sample counts --------
 * vr_gather_flux and vr_gather_paths give every primitive the same K and say nothing of the error.  Sample k of primitive
 * i is a pure function of (seed, i, k) and lives in chunks of 64 with their own engines, so "64 more samples for these
 * primitives only" is exact: nothing already summed is redone.  Two layers.
 * Spec     vr_gather_spec says what a sample is.  paths == 0: vr_gather_flux's sample (cosinePower, mode, emission; the
 *          other fields are not read).  paths == 1: vr_gather_paths's (cosinePower, reflection, maxBounces, reflectivity or
 *          reflectivityScalar); mode must be VR_GATHER_NORMAL and emission NULL.  Pointers are DEVICE memory in the _device
 *          forms and HOST memory in the others.
 * Sums     vr_gather_sums*: for the primitive range and chunks [chunkFirst, chunkFirst + chunks), that is samples
 *          [64 chunkFirst, 64 (chunkFirst + chunks)), of a call of `budget` samples:
 *            sum[i - primFirst]   = sum_k q(w_k)    the exact int64 sum vr_gather_flux / vr_gather_paths divide, q with
 *                                                   wmax(budget);
 *            sumSq[i - primFirst] = sum_k q2(w_k)   q2(w) = 0 for a weight that is not positive, otherwise
 *                                                   (int64)(wc * wc * 2^28 + 0.5) in double, wc = min(w, wmax(budget), 2048).
 *          Outputs are overwritten.  Over chunks [0, K / 64) with budget K, (float)((double)sum / 2^40 / K) has the bits of
 *          the fixed-K call; sums over adjacent chunk ranges add.  budget sums of q2 stay within 2^61.
 * Error    from S1 = sum, S2 = sumSq over K samples, in double, one IEEE operation each in this order, no contraction:
 *            m1 = (double)S1 * 2^-40 / K;  m2 = (double)S2 * 2^-28 / K;  v = m2 - m1 * m1, 0 unless v > 0;
 *            se2 = v / (K - 1);  stdErr = (float)sqrt(se2): the standard error of the mean m1.
 *          converged(rel, abs): se2 <= tol * tol with tol = max((double)rel * m1, (double)abs); rel == abs == 0 means
 *          never.  A primitive whose samples so far all weigh 0 is converged at minSamples under any positive target: the
 *          call cannot know better.  The relative target is on the primitive's own mean.
 * Adaptive vr_gather_adaptive*: minSamples = 64 c0, maxSamples = minSamples 2^R.  wmax = wmax(maxSamples) in every round.
 *          Round 0: every primitive of the range runs chunks [0, c0), K = minSamples.  After a round every primitive still
 *          listed is tested at its K; a converged one gets flux = (float)((double)S1 / 2^40 / K), stdErr, samplesUsed = K
 *          and leaves the list.  Round r >= 1: the listed primitives run chunks [c0 2^(r-1), c0 2^r), K doubles, the sums
 *          are accumulated.  It stops when the list is empty or K == maxSamples; primitives still listed then get their
 *          outputs at maxSamples, and info->unconverged counts those that fail the test there.  info->rounds: rounds run;
 *          info->totalSamples: the sum of samplesUsed over the range.  Weights at most wmax(maxSamples) — every NORMAL
 *          weight — give flux[i] the bits of the fixed-K call at K = samplesUsed[i].
 *          A pure function of scene, vr_set_rng_seed, vr_set_max_boundary_hits and arguments: exact sums and per-primitive
 *          decisions, the same bits for any split of the primitive range over calls and any launch shape.
 * Refused, outputs untouched and the context usable, message in vr_last_error:
 *   VR_E_INVALID  what the fixed-K call of the spec refuses at samples = budget / maxSamples (the samples x g <= 2^22
 *                 rule included); paths not 0 / 1; paths == 1 with a mode other than VR_GATHER_NORMAL or with an emission
 *                 table; 64 (chunkFirst + chunks) > budget; minSamples not a positive multiple of 64; maxSamples not
 *                 minSamples times a power of two; a target that is negative or NaN; a null spec, sum, sumSq, flux or info.
 *                 stdErr and samplesUsed may be NULL.  primCount == 0 is VR_OK after the checks.
 *   VR_E_STATE    as vr_gather_flux_device.
 * Streams, work buffers and "changes nothing of a finished apply": as vr_gather_flux_device.  The adaptive call reads ONE
 * word per round, the next list's length; the work buffers (two int64 arrays, two lists, a few words) grow on demand.
 *
 * sum, sumSq: DEVICE, primCount int64; flux, stdErr: DEVICE, primCount floats; samplesUsed: DEVICE, primCount uint32;
 * info: HOST */
typedef struct vr_gather_spec {
  float cosinePower;
  uint32_t mode;             /* VR_GATHER_NORMAL / VR_GATHER_SOURCE */
  const float *emission;     /* NULL or vr_num_primitives floats by original id (paths == 0) */
  uint32_t paths;            /* 0: vr_gather_flux's sample; 1: vr_gather_paths's */
  uint32_t reflection;       /* VR_GATHER_REFLECT_* (paths == 1) */
  uint32_t maxBounces;
  const float *reflectivity; /* NULL (reflectivityScalar counts) or vr_num_primitives floats by original id */
  float reflectivityScalar;
} vr_gather_spec;
typedef struct vr_gather_adaptive_info {
  uint32_t rounds;
  uint32_t unconverged;
  uint64_t totalSamples;
} vr_gather_adaptive_info;
int vr_gather_sums_device(vr_context *ctx, const vr_gather_spec *spec, uint32_t primFirst, uint32_t primCount,
                          uint32_t chunkFirst, uint32_t chunks, uint32_t budget, int64_t *sum, int64_t *sumSq, void *stream);
/* the same from and to host arrays */
int vr_gather_sums(vr_context *ctx, const vr_gather_spec *spec, uint32_t primFirst, uint32_t primCount, uint32_t chunkFirst,
                   uint32_t chunks, uint32_t budget, int64_t *sum, int64_t *sumSq);
int vr_gather_adaptive_device(vr_context *ctx, const vr_gather_spec *spec, uint32_t primFirst, uint32_t primCount,
                              uint32_t minSamples, uint32_t maxSamples, float relTarget, float absTarget, float *flux,
                              float *stdErr, uint32_t *samplesUsed, vr_gather_adaptive_info *info, void *stream);
/* the same from and to host arrays */
int vr_gather_adaptive(vr_context *ctx, const vr_gather_spec *spec, uint32_t primFirst, uint32_t primCount,
                       uint32_t minSamples, uint32_t maxSamples, float relTarget, float absTarget, float *flux, float *stdErr,
                       uint32_t *samplesUsed, vr_gather_adaptive_info *info);
/* ---- angular gather (not in the reference): a path weighed by tabulated source radiance, sticking and yield -------------
 * vr_gather_paths knows one physics: a power-cosine source, a constant reflectivity, a sample that counts 1 whatever its
 * angle of incidence.  These calls take up to three tabulated ANGULAR LAWS and are otherwise vr_gather_paths bit for bit:
 * scene, range, o_i, m_i, sample numbering, chunk engines, initial direction, segments, wall budget, ends, q(), q2(), wmax,
 * the sums and the final division.
 * Law      M float32 values, 2 <= M <= 256, read as the piecewise-linear function of a cosine x in [0, 1] with nodes at
 *          x_k = k / (M - 1).  The look-up law(t, M, x), float32, one IEEE operation per step, no contraction:
 *            xs = min(max(x, 0), 1) * (float)(M - 1);  k = min((int)xs, M - 2);  f = xs - (float)k;
 *            value = t[k] + f * (t[k + 1] - t[k]).
 *          A NaN x reads as 0.  Host, device and numpy float32 agree bit for bit.  A law whose table is NULL is absent.
 * sourceLaw        L(c): the source's radiance as a function of c = u . w, relative to a Lambertian source: the forward
 *                  source has the direction density L(c) c / Z per solid angle; L = c^(n - 1) is the power cosine.  The
 *                  library normalises on the host, in double, by exact integration of the interpolant: 3-D
 *                  Z = 2 pi int_0^1 L(c) c dc; 2-D Z = 2 int_0^1 L(c) c / sqrt(1 - c^2) dc (per segment, L = a + b c: the
 *                  antiderivative -a sqrt(1 - c^2) + b (asin c - c sqrt(1 - c^2)) / 2).  g_L = (float)(pi / Z) in 3-D,
 *                  (float)(2 / Z) in 2-D.  A path that reaches the source plane with c_end > 0 weighs
 *                  (g_L * law(L, c_end)) * T in place of g c_end^(n - 1) * T.  Entries finite and >= 0, not all 0;
 *                  spec->cosinePower must be 1.
 * reflectivityLaw  R(mu): the share that is NOT absorbed, as a function of mu = n_j . (the direction the path LEAVES the
 *                  vertex along) — unprojected, after the reflection, (n.x d.x + n.y d.y) + n.z d.z — the forward particle's
 *                  cosine of incidence.  For a mirror that is the arriving ray's cosine; for a DIFFUSE vertex the cosine of
 *                  the direction just drawn, the adjoint of "sticks by its incidence, re-emits by the cosine law".
 *                  T <- (T * rho[j]) * R(mu): two multiplies in this order; T == 0 after either ends the path
 *                  (VR_GATHER_END_ABSORBED).  Entries in [0, 1].
 * yieldLaw         Y(mu0), mu0 = m_i . w_0 of the sample's INITIAL direction against the starting primitive's own normal.
 *                  One more multiply, last: w = ((g_L L(c_end) or g c_end^(n - 1)) * T) * Y(mu0).  Entries finite and >= 0;
 *                  they may exceed 1.
 * Bounds   wbound = (g_L max L or g) max Y.  A call with samples x wbound > 2^22 is refused as samples x g is; the
 *          per-sample variance is at most F (wbound - F).  The source law WEIGHS the samples, it does not place them: a
 *          narrow L has the variance g_L max L says it has (vr_gather_angular_adaptive's stdErr shows it).
 * Identities  laws == NULL or all three tables NULL: the bits of vr_gather_paths / vr_gather_sums / vr_gather_adaptive /
 *          vr_debug_gather_path.  All-ones tables of any M: those bits too (g_L is exactly 1.0f).  R = 0.5 everywhere with
 *          reflectivity rho: the bits of vr_gather_paths at rho / 2.
 * Coned-cosine reflection is not offered: its kernel p(w_out | w_in) is not symmetric (the cone's opening depends on the
 * incidence), so a backward path cannot reverse it step by step as it reverses a mirror or a Lambertian re-emission.
 * spec: a vr_gather_spec with paths == 1, mode VR_GATHER_NORMAL and emission NULL (anything else is refused);
 * spec->reflectivity is DEVICE memory in the _device forms and HOST memory in the others.  The tables of vr_gather_laws are
 * always HOST pointers: they are tiny, validated and normalised on the host, and copied at the call.
 * Refused, outputs untouched and the context usable, message in vr_last_error:
 *   VR_E_INVALID  what the matching entry point without laws refuses; a count outside 2 .. 256; an entry outside its
 *                 law's range (the message names the law and the lowest such index); a source law that is all 0, or with
 *                 cosinePower != 1; samples (budget, maxSamples) x wbound > 2^22.
 *   VR_E_STATE    as vr_gather_flux_device.
 * Streams, work buffers and "changes nothing of a finished apply": as the matching entry point without laws.
 * Outputs as those of vr_gather_paths*, vr_gather_sums*, vr_gather_adaptive* and vr_debug_gather_path */
typedef struct vr_gather_laws {
  const float *sourceLaw;       /* NULL or sourceCount HOST floats */
  uint32_t sourceCount;
  const float *reflectivityLaw; /* NULL or reflectivityCount HOST floats */
  uint32_t reflectivityCount;
  const float *yieldLaw;        /* NULL or yieldCount HOST floats */
  uint32_t yieldCount;
} vr_gather_laws;
int vr_gather_angular_device(vr_context *ctx, const vr_gather_spec *spec, const vr_gather_laws *laws, uint32_t primFirst,
                             uint32_t primCount, uint32_t samples, float *out, void *stream);
int vr_gather_angular(vr_context *ctx, const vr_gather_spec *spec, const vr_gather_laws *laws, uint32_t primFirst,
                      uint32_t primCount, uint32_t samples, float *out);
int vr_gather_angular_sums_device(vr_context *ctx, const vr_gather_spec *spec, const vr_gather_laws *laws, uint32_t primFirst,
                                  uint32_t primCount, uint32_t chunkFirst, uint32_t chunks, uint32_t budget, int64_t *sum,
                                  int64_t *sumSq, void *stream);
int vr_gather_angular_sums(vr_context *ctx, const vr_gather_spec *spec, const vr_gather_laws *laws, uint32_t primFirst,
                           uint32_t primCount, uint32_t chunkFirst, uint32_t chunks, uint32_t budget, int64_t *sum,
                           int64_t *sumSq);
int vr_gather_angular_adaptive_device(vr_context *ctx, const vr_gather_spec *spec, const vr_gather_laws *laws,
                                      uint32_t primFirst, uint32_t primCount, uint32_t minSamples, uint32_t maxSamples,
                                      float relTarget, float absTarget, float *flux, float *stdErr, uint32_t *samplesUsed,
                                      vr_gather_adaptive_info *info, void *stream);
int vr_gather_angular_adaptive(vr_context *ctx, const vr_gather_spec *spec, const vr_gather_laws *laws, uint32_t primFirst,
                               uint32_t primCount, uint32_t minSamples, uint32_t maxSamples, float relTarget, float absTarget,
                               float *flux, float *stdErr, uint32_t *samplesUsed, vr_gather_adaptive_info *info);
/* ONE path as vr_debug_gather_path records it (spec->reflectivity: NULL or HOST floats), weighed by the laws: the leaving
 * direction and the normal of every vertex give its mu, *throughput and *weight are the path's */
int vr_debug_gather_angular_path(vr_context *ctx, const vr_gather_spec *spec, const vr_gather_laws *laws, uint32_t prim,
                                 uint32_t sample, uint32_t maxVertices, uint32_t *vertexIds, float *vertexData,
                                 uint32_t *numVertices, uint32_t *end, float *finalDirection3, float *throughput,
                                 float *weight);
/* ---- energy gather (not in the reference): an ion's energy lost along a path, a yield by the arrival energy -------------
 * vr_gather_angular weighs a path by angles.  An ion-enhanced etch or sputter yield also depends on the ENERGY the ion
 * arrives with: it leaves the source with E0 and keeps a share eps(mu) of its energy at every reflection.  A backward path
 * can carry that exactly because the loss is multiplicative: the ion arrives with E0 prod_j eps(mu_j), a product that does
 * not depend on the order the vertices are visited in.  These calls are vr_gather_angular with one more multiply at the
 * tail and are otherwise that call bit for bit: samples, chunk engines, segments, walls, ends, q(), q2(), wmax, the sums
 * and the final division.
 * Tables   vr_gather_energy holds HOST tables, read by vr_gather_angular's look-up law(t, M, x):
 *   energyYield      Y_E(e), REQUIRED, 2 .. 256 entries finite and >= 0, read at e in [0, 1].
 *   energyMax        the energy that e = 1 stands for; finite, > 0.
 *   sourceQuantiles  NULL, or 2 .. 256 entries finite and >= 0: the source's inverse CDF Q(u), read at u.
 *   sourceEnergy     used where sourceQuantiles is NULL: a monoenergetic source.  Finite, >= 0.
 *   retentionLaw     NULL (no loss), or 2 .. 256 entries in [0, 1]: eps(mu) at the mu of reflectivityLaw,
 *                    mu = n_j . (the direction the path LEAVES the vertex along).
 *   energyCut        1 or 0 (below).
 * Sample   Per sample k of primitive i, float32, one IEEE operation per step in this order, no contraction:
 *            key = tea8(i, (seed ^ "PATH") + k), the key of the DIFFUSE draws;
 *            u = (tea8(key, 0x454E5247) >> 8) * 2^-24   (the counter is "ENRG"; the bounce counters stop at 131071);
 *            E0 = sourceQuantiles ? law(Q, MQ, u) : sourceEnergy;  P = 1;
 *            at every front-side hit after which the path goes on (both of T's multiplies passed):
 *              P = P * law(eps, Meps, mu);
 *            e = (E0 * P) / energyMax   — the arrival energy in table units, the product first;
 *            w = w_angular * law(Y_E, MY, e)   — the last multiply.
 * Bounds   wbound = wbound_angular max Y_E; samples (budget, maxSamples) x wbound > 2^22 is refused.
 * Cut      Z0: the number of leading entries of energyYield equal to 0.  With energyCut and Z0 >= 2, and
 *          xs = min(max(e, 0), 1) * (float)(MY - 1) — the look-up's own xs — a path ends with VR_GATHER_END_ENERGY, weight
 *          0, as soon as xs < (float)(Z0 - 1).  The test is made once before the walk (P = 1: such a sample is not walked
 *          at all) and after every update of P.  eps <= 1 and rounding is monotone, so e never rises, and every e with
 *          xs < Z0 - 1 reads exactly 0: flux, sums and sums of squares have the same bits with the cut on and off.
 * Identities  energy == NULL: the bits of the vr_gather_angular* call.  An all-ones energyYield of any M, with anything in
 *          the other fields: those bits too.  With reflectivityScalar 1, no yieldLaw, sourceEnergy = energyMax = 1,
 *          energyYield = {0, 1} and retentionLaw = R: the bits of vr_gather_angular with reflectivityLaw = R (P is then that
 *          call's T multiply for multiply, and {0, 1} read at e returns e).
 * Refused, outputs untouched and the context usable, message in vr_last_error:
 *   VR_E_INVALID  what the matching vr_gather_angular* call refuses; a NULL energyYield; a count outside 2 .. 256; an
 *                 entry outside its table's range (the message names the table and the lowest such index); energyMax not
 *                 finite or not > 0; a negative or non-finite sourceEnergy; energyCut other than 0 or 1;
 *                 samples x wbound > 2^22.
 *   VR_E_STATE    as vr_gather_flux_device.
 * Streams, work buffers and "changes nothing of a finished apply": as the matching vr_gather_angular* call.
 * Outputs as those of vr_gather_angular*.  Energy in vr_gather_species*, a stochastic spread of the retained energy and
 * yields of two variables Y(theta, E) are not offered */
#define VR_GATHER_END_ENERGY 7 /* the arrival energy entered the zero region of energyYield (the cut) */
/* (a struct tag alone, no typedef: vr_gather_energy is also the name of the host entry point) */
struct vr_gather_energy {
  const float *energyYield; /* energyYieldCount HOST floats */
  uint32_t energyYieldCount;
  float energyMax;
  const float *sourceQuantiles; /* NULL or sourceQuantilesCount HOST floats */
  uint32_t sourceQuantilesCount;
  float sourceEnergy;
  const float *retentionLaw; /* NULL or retentionCount HOST floats */
  uint32_t retentionCount;
  uint32_t energyCut;
};
int vr_gather_energy_device(vr_context *ctx, const vr_gather_spec *spec, const vr_gather_laws *laws,
                            const struct vr_gather_energy *energy, uint32_t primFirst, uint32_t primCount, uint32_t samples,
                            float *out, void *stream);
int vr_gather_energy(vr_context *ctx, const vr_gather_spec *spec, const vr_gather_laws *laws, const struct vr_gather_energy *energy,
                     uint32_t primFirst, uint32_t primCount, uint32_t samples, float *out);
int vr_gather_energy_sums_device(vr_context *ctx, const vr_gather_spec *spec, const vr_gather_laws *laws,
                                 const struct vr_gather_energy *energy, uint32_t primFirst, uint32_t primCount, uint32_t chunkFirst,
                                 uint32_t chunks, uint32_t budget, int64_t *sum, int64_t *sumSq, void *stream);
int vr_gather_energy_sums(vr_context *ctx, const vr_gather_spec *spec, const vr_gather_laws *laws,
                          const struct vr_gather_energy *energy, uint32_t primFirst, uint32_t primCount, uint32_t chunkFirst,
                          uint32_t chunks, uint32_t budget, int64_t *sum, int64_t *sumSq);
int vr_gather_energy_adaptive_device(vr_context *ctx, const vr_gather_spec *spec, const vr_gather_laws *laws,
                                     const struct vr_gather_energy *energy, uint32_t primFirst, uint32_t primCount,
                                     uint32_t minSamples, uint32_t maxSamples, float relTarget, float absTarget, float *flux,
                                     float *stdErr, uint32_t *samplesUsed, vr_gather_adaptive_info *info, void *stream);
int vr_gather_energy_adaptive(vr_context *ctx, const vr_gather_spec *spec, const vr_gather_laws *laws,
                              const struct vr_gather_energy *energy, uint32_t primFirst, uint32_t primCount, uint32_t minSamples,
                              uint32_t maxSamples, float relTarget, float absTarget, float *flux, float *stdErr,
                              uint32_t *samplesUsed, vr_gather_adaptive_info *info);
/* ONE path as vr_debug_gather_angular_path records it, with its energy: energyOut4 (NULL, or 4 floats) = {u, E0, P, e}; with
 * energy == NULL it is that call and energyOut4 is left alone.  A sample the cut ended before its walk has one vertex; a
 * vertex the cut ended the path on keeps its leaving direction — the one its retention was read at — where every other
 * last vertex has NaN */
int vr_debug_gather_energy_path(vr_context *ctx, const vr_gather_spec *spec, const vr_gather_laws *laws,
                                const struct vr_gather_energy *energy, uint32_t prim, uint32_t sample, uint32_t maxVertices,
                                uint32_t *vertexIds, float *vertexData, uint32_t *numVertices, uint32_t *end,
                                float *finalDirection3, float *throughput, float *weight, float *energyOut4);
/* ---- species gather (not in the reference): several species weighed along one set of traced paths ----------------------
 * A process step has two or three ion species, or one whose arrivals feed several yields.  Each is a vr_gather_angular
 * call, and every call walks the same paths again: the samples are a pure function of (seed, primitive, sample), the
 * mirror direction follows from the normal, the DIFFUSE draw from (seed, primitive, sample, bounce).  What differs per
 * species is a handful of multiplies along the path.  These calls walk once for up to VR_GATHER_MAX_SPECIES species.
 * Species  A call has S species, 1 <= S <= VR_GATHER_MAX_SPECIES.  Species s is specs[s] plus, where laws is not NULL,
 *          laws[s], and means exactly what vr_gather_angular means by that pair (vr_gather_paths where it has no law).
 *          Shared by all species: paths == 1, mode == VR_GATHER_NORMAL, emission == NULL, reflection, maxBounces.
 *          Per species: cosinePower (1 where it has a source law), reflectivity or reflectivityScalar, the three laws.
 * Path     The shared path is sample k of primitive i exactly as vr_gather_paths starts and walks it.  Every species
 *          starts alive with T_s = 1.  At a geometry hit of primitive j, in vr_gather_paths's order:
 *            1. a back side ends the path for every species;
 *            2. bounces >= maxBounces ends the path for every species;
 *            3. for each species still alive T_s <- T_s * rho_s[j]; T_s == 0 makes that species dead;
 *            4. if no species is alive the path ends;
 *            5. otherwise the leaving direction is formed ONCE (the mirror direction, or the counter draw of this bounce);
 *            6. for each living species with a reflectivity law T_s <- T_s * R_s(mu); T_s == 0 makes it dead;
 *            7. if none is alive the path ends; otherwise it restarts from the hit point and the bounce is counted.
 *          A dead species weighs exactly 0 for this sample: it is not weighed from a T of 0.  The path's geometry is that
 *          of the species that lives longest; up to its own death every species sees its own single-species path.
 * Weight   At the path's tail every living species is weighed by vr_gather_angular's rule with its own g, cosinePower,
 *          g_L, laws and T_s and the shared c_end and mu0, then q() with wmax(samples) into its own exact int64 sum.
 * Result   out[s * primCount + (i - primFirst)].  Row s has the BITS of the single-species call of species s —
 *          vr_gather_angular(specs[s], laws[s]), vr_gather_paths without laws — for every s, S, order of the species,
 *          split of the primitive range over calls and launch shape.  That identity is the specification.
 * Sums     vr_gather_species_sums*: sum and sumSq as vr_gather_angular_sums gives them, numSpecies x primCount each, row s
 *          that call's for species s bit for bit.  They are the layer under the adaptive call below.
 * Bounds   samples (budget) x wbound_s <= 2^22 for every species, wbound as vr_gather_angular's.
 * Refused, outputs untouched and the context usable, message in vr_last_error — every message about one species names it
 * ("... species 2: ..."):
 *   VR_E_INVALID  specs NULL; numSpecies 0 or above VR_GATHER_MAX_SPECIES; a species whose paths is not 1, whose mode is
 *                 not VR_GATHER_NORMAL or that has an emission table; a species whose reflection or maxBounces differs from
 *                 species 0's (the first such species); what vr_gather_angular refuses of a species' spec and laws — the
 *                 samples x wbound rule, a law's count or entries, a reflectivity outside [0, 1] (a table is checked on
 *                 the device, one word per species back: the first species with a bad entry and its lowest such index);
 *                 out, sum or sumSq null with primCount > 0; 64 (chunkFirst + chunks) > budget.
 *                 primCount == 0 is VR_OK after the checks.
 *   VR_E_STATE    as vr_gather_flux_device.
 * Streams, work buffers (numSpecies of each of the gather's) and "changes nothing of a finished apply": as
 * vr_gather_angular_device.  vr_debug_gather_angular_path with species s's spec and laws returns that species' prefix of
 * the shared path.
 * specs: numSpecies structs; laws: NULL or numSpecies structs (HOST tables, as vr_gather_angular); specs[s].reflectivity:
 * DEVICE memory in the _device forms, HOST memory in the others; out: numSpecies x primCount floats; sum, sumSq:
 * numSpecies x primCount int64 */
#define VR_GATHER_MAX_SPECIES 4u
int vr_gather_species_device(vr_context *ctx, const vr_gather_spec *specs, const vr_gather_laws *laws, uint32_t numSpecies,
                             uint32_t primFirst, uint32_t primCount, uint32_t samples, float *out, void *stream);
/* the same from and to host arrays */
int vr_gather_species(vr_context *ctx, const vr_gather_spec *specs, const vr_gather_laws *laws, uint32_t numSpecies,
                      uint32_t primFirst, uint32_t primCount, uint32_t samples, float *out);
int vr_gather_species_sums_device(vr_context *ctx, const vr_gather_spec *specs, const vr_gather_laws *laws, uint32_t numSpecies,
                                  uint32_t primFirst, uint32_t primCount, uint32_t chunkFirst, uint32_t chunks, uint32_t budget,
                                  int64_t *sum, int64_t *sumSq, void *stream);
int vr_gather_species_sums(vr_context *ctx, const vr_gather_spec *specs, const vr_gather_laws *laws, uint32_t numSpecies,
                           uint32_t primFirst, uint32_t primCount, uint32_t chunkFirst, uint32_t chunks, uint32_t budget,
                           int64_t *sum, int64_t *sumSq);
/* ---- species gather to a target error (not in the reference): per-species adaptive sampling along one walk ----------------
 * A process step wants each of its species to a target error, not to a fixed K.  vr_gather_species at the worst
 * primitive's K wastes samples; numSpecies vr_gather_angular_adaptive calls walk the same paths again.  These calls run the
 * rounds of vr_gather_adaptive once, for all species, and let every species of every primitive stop on its own.
 * Species  specs[s] plus laws[s], exactly as vr_gather_species takes them, 1 <= numSpecies <= VR_GATHER_MAX_SPECIES.
 * Targets  relTargets[s], absTargets[s]: HOST arrays of numSpecies floats, the targets of species s.
 * Rounds   minSamples, maxSamples, the chunk ranges of the rounds and wmax = wmax(maxSamples) in every round are those of
 *          vr_gather_adaptive.  Every listed primitive carries a MASK of the species still sampling there; in round 0 every
 *          primitive of the range is listed with all species.  After a round, at its K, every species in a listed
 *          primitive's mask is tested by converged(relTargets[s], absTargets[s]) on its own two sums:
 *            - one that converges gets flux, stdErr and samplesUsed at that K and leaves the mask; its sums are never
 *              touched again;
 *            - a primitive leaves the list when its mask is empty;
 *            - at K == maxSamples every species still in a mask gets its outputs, and info->unconverged[s] counts those of
 *              species s that fail the test there.
 *          In a later round a primitive's paths start with alive = its mask.  A species outside the mask is dead from the
 *          start: it is weighed nowhere, and it does not keep the shared path going.
 * Result   flux, stdErr, samplesUsed: [s * primCount + (i - primFirst)].  Row s of each has the BITS of
 *          vr_gather_angular_adaptive (vr_gather_adaptive where the species has no law) called with specs[s], laws[s],
 *          relTargets[s], absTargets[s] and the same minSamples / maxSamples — for every s and numSpecies, every order of
 *          the species, every choice of the OTHER species and their targets, every split of the primitive range over calls
 *          and every launch shape.  That identity is the specification.  It holds because up to the vertex where species s
 *          dies the shared path is its own path (vr_gather_species), and its sums take exactly the chunks its own call
 *          would have run: it is in the mask in exactly the rounds its own call lists the primitive.
 * info     rounds: the rounds run, the maximum of the species' own calls' rounds.  unconverged[s], totalSamples[s]: what
 *          the call of species s alone reports.  walkedSamples: the sum over the primitives of the largest samplesUsed
 *          among their species — the samples actually walked; at most the sum of totalSamples, and below it wherever two
 *          species of a primitive share a round.
 * numSpecies == 1 is vr_gather_angular_adaptive itself.
 * Refused, outputs untouched and the context usable, message in vr_last_error — every message about one species names it:
 *   VR_E_INVALID  what vr_gather_species refuses at samples = maxSamples; what vr_gather_adaptive refuses of minSamples and
 *                 maxSamples; relTargets or absTargets NULL; a target of a species that is negative or NaN ("... species 2:
 *                 ..."); flux or info NULL.  stdErr and samplesUsed may be NULL.  primCount == 0 is VR_OK after the checks.
 *   VR_E_STATE    as vr_gather_flux_device.
 * Streams and "changes nothing of a finished apply": as vr_gather_adaptive_device.  The host waits once per round, for five
 * words: the next list's length and, per species, the primitives it still samples in.  Work buffers: numSpecies x primCount
 * of each sum, two lists with their masks, a few words per round; they grow on demand.
 * flux, stdErr: numSpecies x primCount floats, samplesUsed: numSpecies x primCount uint32 — DEVICE memory in the _device
 * form (as specs[s].reflectivity), HOST memory in the other; relTargets, absTargets, info: HOST */
typedef struct vr_gather_species_adaptive_info {
  uint32_t rounds;
  uint32_t unconverged[VR_GATHER_MAX_SPECIES];
  uint64_t totalSamples[VR_GATHER_MAX_SPECIES];
  uint64_t walkedSamples;
} vr_gather_species_adaptive_info;
int vr_gather_species_adaptive_device(vr_context *ctx, const vr_gather_spec *specs, const vr_gather_laws *laws, uint32_t numSpecies,
                                      uint32_t primFirst, uint32_t primCount, uint32_t minSamples, uint32_t maxSamples,
                                      const float *relTargets, const float *absTargets, float *flux, float *stdErr,
                                      uint32_t *samplesUsed, vr_gather_species_adaptive_info *info, void *stream);
/* the same from and to host arrays */
int vr_gather_species_adaptive(vr_context *ctx, const vr_gather_spec *specs, const vr_gather_laws *laws, uint32_t numSpecies,
                               uint32_t primFirst, uint32_t primCount, uint32_t minSamples, uint32_t maxSamples,
                               const float *relTargets, const float *absTargets, float *flux, float *stdErr, uint32_t *samplesUsed,
                               vr_gather_species_adaptive_info *info);
/* ---- radiosity solve (not in the reference): the steady-state flux of a diffusely re-emitting species ------------------
 * vr_gather_flux with an emission table is one radiosity iteration, and its walks are a constant of the scene.  These
 * calls record them once — a link table — and iterate over the table on the device without walking again.
 * Scene, seed, sample k of primitive i, its direction, its walk and "front side" are exactly those of vr_gather_flux in
 * VR_GATHER_NORMAL mode over the whole scene (primFirst = 0, primCount = vr_num_primitives).
 * Link table for (samples = K, cosinePower = n), per primitive i:
 *   direct[i]   = sum_k q(w_k) over the samples that reached the source: the int64 sum of a vr_gather_flux call without
 *                 emission.
 *   link[i][k]  = the original id j of the primitive sample k hit on its front side; -1 for everything else — a
 *                 back-side hit, a miss with c <= 0, a sample that left through an IGNORE wall or was stopped by the wall
 *                 budget, and a sample that reached the source.
 * One iteration with emission table e (float32 per primitive):
 *   G(e)[i] = result(direct[i] + sum_{k: link >= 0} q(e[link[i][k]]), K), q and result those of vr_gather_flux with
 *   wmax(K).  Exact int64 sums: G(e) has the bits of vr_gather_flux(0, N, K, n, VR_GATHER_NORMAL, e).
 * Solve with reflectivity rho (one float32 per primitive or a scalar, 0 <= rho <= 1; for sticking s, rho = 1 - s):
 *   F_0 = G(nothing), the direct flux;  e_t[j] = rho[j] * F_{t-1}[j] (one float32 multiply);  F_t = G(e_t);
 *   r_t = max_i |F_t[i] - F_{t-1}[i]| (a float32 subtraction; the maximum is taken over the bit patterns, so order cannot
 *   show).  The solve stops at the first t >= 1 with r_t <= tolerance, or at t = maxIterations; maxIterations = 0 returns
 *   F_0.  It returns F_t, t and r_t (0 for t = 0).  A pure function of scene, vr_set_rng_seed, vr_set_max_boundary_hits, K,
 *   n, rho, tolerance and maxIterations: grid shape and the way the host batches iterations cannot show.
 * Units are the gather's: the SOURCE-normalised INCOMING flux (what a diffuse particle credits), not that flux times the
 * sticking.
 * Memory: the table takes 4 x (N rounded up to 64) x K bytes plus 8 N for the sums, in buffers the context keeps until
 *   vr_radiosity_free_links or vr_destroy; vr_radiosity_link_bytes says how much before it is built.  Its layout is
 *   private.  A table that cannot be allocated is refused with VR_E_HIP; the context stays usable and NO table is resident
 *   afterwards (building replaces: the previous table is gone as soon as the arguments have been accepted).
 * vr_radiosity_links_device builds or replaces the table.  Refused as vr_gather_flux_device in VR_GATHER_NORMAL mode
 *   (VR_E_INVALID: samples == 0, cosinePower not finite or < 1, samples x g beyond 2^22; VR_E_STATE: as
 *   vr_cast_rays_device).  Changes nothing of a finished apply; the next apply gives the bits it would have given.
 * A table remembers the scene build, the boundary conditions, the source direction, vr_set_max_boundary_hits, the rng
 *   seed, K and n it was built from.  Every call that reads it is VR_E_STATE, with a message that says which of them has
 *   changed, once they no longer match the settings in force — and VR_E_STATE when there is no table.
 *   vr_radiosity_resident: 1 if a table for (samples, cosinePower) is resident and matches, else 0.
 * vr_radiosity_solve_device: reflectivity NULL (reflectivityScalar counts) or DEVICE, N floats by original id; out:
 *   DEVICE, N floats; iterations / residual: NULL or host words.  The host waits for the residuals.  Refused, out
 *   untouched and the context usable: VR_E_INVALID for a reflectivity that is NaN, negative or above 1 (checked on the
 *   device, ONE word back; the message names the lowest such index), a tolerance that is negative or NaN (0 is allowed:
 *   the solve then runs until the flux stops changing bit for bit, or maxIterations), out null, a pointer that is not
 *   device memory of ctx's device; VR_E_STATE as above.
 * vr_radiosity_solve: the same from and to host arrays.  vr_radiosity_direct_device: F_0 from the table.
 * vr_debug_radiosity_links: links first .. first + count - 1 of primitive prim as ORIGINAL ids, into host memory.
 * vr_debug_radiosity_time_iterations: a measurement — `count` iteration kernels with a scalar reflectivity launched back
 *   to back between two events, converged or not, with (nontemporal != 0) or without non-temporal loads for the link
 *   stream; *msPerIteration is the elapsed time over count.  It returns no flux. */
uint64_t vr_radiosity_link_bytes(const vr_context *ctx, uint32_t samples);
int vr_radiosity_links_device(vr_context *ctx, uint32_t samples, float cosinePower, void *stream);
int vr_radiosity_resident(const vr_context *ctx, uint32_t samples, float cosinePower);
int vr_radiosity_solve_device(vr_context *ctx, const float *reflectivity, float reflectivityScalar, float tolerance,
                              uint32_t maxIterations, float *out, uint32_t *iterations, float *residual, void *stream);
int vr_radiosity_solve(vr_context *ctx, const float *reflectivity, float reflectivityScalar, float tolerance,
                       uint32_t maxIterations, float *out, uint32_t *iterations, float *residual);
int vr_radiosity_direct_device(vr_context *ctx, float *out, void *stream);
int vr_debug_radiosity_links(vr_context *ctx, uint32_t prim, uint32_t first, uint32_t count, int32_t *links);
int vr_debug_radiosity_time_iterations(vr_context *ctx, float reflectivityScalar, uint32_t count, int nontemporal,
                                       float *msPerIteration);
int vr_radiosity_free_links(vr_context *ctx);
/* ---- flux statistics (not in the reference): per-primitive hit counts and the Monte-Carlo error of the flux ----------
 * vr_set_flux_statistics(on != 0): every later apply() keeps, for each particle and alongside its data label 0 (the flux
 * label of every built-in model), two more int64 sums per primitive:
 *   hits[i]   the number of credits to label 0 of primitive i — the closest primitive and every overlapping neighbour disk
 *             count one each — in units of ONE;
 *   sumsq[i]  the sum over those credits of (double)v * (double)v, v the float handed to credit(0, v) (after WDIST
 *             weighting), quantised like the flux: * 2^VR_FLUX_FRAC_BITS + 0.5.
 * Exact integer sums like the flux: independent of grid, batch split and rank count.  They are planes numData and
 * numData + 1 of the particle, BEHIND its data labels, in the same array: vr_flux_accumulators / vr_bind_flux_accumulators
 * then hold numPrims x (data labels + 2 per particle) words, particle after particle, and vr_apply_sharded all-reduces
 * them with the flux.  vr_num_data and the dataIdx of the flux getters do not change.  Off by default; switching discards
 * the last result and a bound accumulator buffer of the other size.
 *   sigma[i]    = sqrt(max(sumsq[i] - S1[i]^2 / N, 0)), S1 the raw label-0 sum, N the rays of the WHOLE apply (with
 *                 vr_set_ray_range / vr_apply_sharded: of all shards together, so summed accumulators give the apply's value)
 *   relative[i] = sigma[i] / S1[i], +inf where S1[i] == 0; the same for every normalisation.  The absolute error is in raw
 *                 flux units.
 * A PER-CREDIT estimator: it ignores the correlation between several credits of one ray to the same primitive
 * ("Flux statistics", has the calibration against the run-to-run scatter).
 * Launches: an absorbing launch (sticking 1 everywhere, unit start weights) keeps its kernel and trace mode — unit
 * weights, hits = sumsq = flux, filled from the flux plane; every other launch runs the extended kernels with the
 * statistics compiled in (modes 0, 4 and, on flat disk scenes without the rare options, 3; no relief modes 6 / 7), a
 * run-time model in a twin of its code object compiled on first use.  With statistics on a particle model may have at
 * most VR_MAX_LABELS - 2 = 2 data labels (refused at prepare).
 * The getters fail (message in vr_last_error) with statistics off, before an apply has finished, with n != numPrims or
 * particleIdx beyond the particle list.  vr_get_flux_sum_squares: acc * 2^-40, exact.  vr_get_flux_error: kind 0
 * relative, 1 absolute, float32, computed on the device in double.  vr_get_flux_error_device: the same floats into DEVICE
 * memory, under vr_get_flux_device's stream rules.                                                                     */
int vr_set_flux_statistics(vr_context *ctx, int on);
int vr_get_hit_counts(vr_context *ctx, uint32_t particleIdx, uint64_t *out, uint32_t n);
int vr_get_flux_sum_squares(vr_context *ctx, uint32_t particleIdx, double *out, uint32_t n);
int vr_get_flux_error(vr_context *ctx, uint32_t particleIdx, int kind, float *out, uint32_t n);
int vr_get_flux_error_device(vr_context *ctx, uint32_t particleIdx, int kind, float *out, uint32_t n, void *stream);
/* geometry-derived values the reference exposes to its tests                */
int vr_get_disk_areas(vr_context *ctx, float *out, uint32_t n);
int vr_get_bounding_box(vr_context *ctx, float *out6 /* min xyz, max xyz, adjusted */);
float vr_get_source_area(vr_context *ctx);
float vr_get_disk_radius(const vr_context *ctx);
int vr_get_neighbor_counts(vr_context *ctx, uint32_t *out, uint32_t n);

/* ---- device accumulators for collectives (multi-GPU) ----------------------
 * The per-primitive accumulator is an int64 fixed-point sum (weight * 2^VR_FLUX_FRAC_BITS),
 * so sums are order-independent and an integer all-reduce is exact.  The
 * pointer is DEVICE memory of `n` int64, in the caller's primitive order; it is
 * valid after vr_apply_finish() until the next launch.  vr_flux_accumulators_from
 * replaces the device contents (e.g. after an all-reduce done elsewhere).    */
#define VR_FLUX_FRAC_BITS 40
int vr_flux_accumulators(vr_context *ctx, void **devPtr, uint32_t *n);
/* ---- the data log (DataLog / AbstractParticle::logData, rayTraceKernel.hpp:131-133, 345) ----------------------
 * A stateful run-time model (vr_register_particle_model_ex) with `static constexpr int kLogRows = R` (1 .. 16) and
 *     template <class Log> __device__ static void log_data(const ModelCtx &, const RayState &s, Log &&log);
 * logs once per ray, right after init and before the source sample: log(row, bin, value) is
 * dataLog.data[row][bin] += value.  The hook draws nothing from the engine and cannot change the state.  The sums are
 * int64 fixed point (value * 2^VR_LOG_FRAC_BITS): exact for counts, 6e-8 resolution, independent of grid, batch
 * split and rank count.  A call with row / bin outside the shape, or a value that is negative, not finite or above
 * 2^15, is dropped and counted.  An entry holds 2^39 (5.5e11) units per apply(), divided by the rank count rounded up
 * to a power of two; beyond that the apply FAILS (VR_E_STATE, TraceInfo.error = 1, "data log overflow").
 *
 * vr_set_data_log_shape: the entries per row (at most 16 rows, 65536 entries in all); rows == 0 clears the shape and
 * nothing is logged.  With a shape set, vr_apply_prepare refuses an apply none of whose particle models has a hook, and
 * a shape with fewer rows than a hook's kLogRows.  Every apply starts from a zeroed log; in a particle list every model
 * with a hook adds to the one log.  vr_apply_sharded all-reduces the log with the flux.
 * vr_get_data_log: the last apply's sums as float(double(sum) * 2^-VR_LOG_FRAC_BITS), rows concatenated (n = all
 * entries); vr_get_data_log_i64: the sums themselves; vr_get_data_log_dropped: the dropped calls.
 * vr_data_log_accumulators: DEVICE memory of n int64 sums for callers that own the collective, valid from
 * vr_apply_prepare until the shape changes; words [n] and [n + 1] behind them are the dropped counter and the overflow
 * flag, so an all-reduce of n + 2 words carries both.                                                          */
#define VR_LOG_FRAC_BITS 24
int vr_set_data_log_shape(vr_context *ctx, const uint32_t *rowSizes, uint32_t rows);
int vr_get_model_log_rows(const vr_context *ctx, int32_t kind, int32_t *rows); /* kLogRows of a particle kind (0: no hook) */
int vr_get_data_log(vr_context *ctx, float *out, uint32_t n);
int vr_get_data_log_i64(vr_context *ctx, int64_t *out, uint32_t n);
int vr_get_data_log_dropped(vr_context *ctx, uint64_t *out);
int vr_data_log_accumulators(vr_context *ctx, void **devPtr, uint32_t *n);
/* Let the caller own the accumulator buffer instead (e.g. a torch int64 tensor
 * handed to torch.distributed/RCCL): DEVICE pointer to n int64; NULL restores
 * the library-owned buffer.  Must stay valid until replaced.  The binding survives
 * vr_set_particle(s) as long as numPrims x data labels is unchanged; a call that changes the
 * number of data labels, and vr_set_disks / vr_set_triangles, drop it (the library's own
 * buffer is used again: bind anew).                                          */
int vr_bind_flux_accumulators(vr_context *ctx, void *devPtr, uint32_t n);
int vr_add_trace_info(vr_context *ctx, const vr_trace_info *other);
/* stream the context launches on (hipStream_t as void*)                      */
void *vr_stream(vr_context *ctx);

/* ---- diagnostics used by the parity tests --------------------------------- */
/* closest hit of explicit rays against {boundary, geometry} (rtcIntersect1 stand-in,
 * rayTraceKernel.hpp:163-167).  geomID: 0 boundary, 1 geometry, -1 miss.     */
int vr_debug_intersect(vr_context *ctx, const float *org, const float *dir,
                       const float *tnear, uint32_t nrays, int32_t *geomID,
                       uint32_t *primID, float *t);
/* Boundary::processHit (rayBoundary.hpp:29-127) for hand-built hits, as the reference's
 * tests/boundaryHit and tests/boundaryHit2D feed it: ray (org, dir) meets wall triangle primID
 * (0..7) at tfar                                                                              */
int vr_debug_process_hit(vr_context *ctx, const float *org, const float *dir, const float *tfar,
                         const uint32_t *primID, uint32_t n, float *outOrg, float *outDir, int32_t *outReflect);
/* first (origin, direction) of global ray indices idx[] for kernel seed `seed`
 * (raySourceRandom.hpp:25-36 after rayTraceKernel.hpp:120-121)               */
int vr_debug_source_sample(vr_context *ctx, const uint64_t *idx, uint32_t n,
                           uint32_t seed, float *org, float *dir);
/* ... for the active stateful model (vr_register_particle_model_ex): its generator's first (origin, direction) and
 * the engine outputs consumed before the trace (init + source sample) of global ray indices idx[]         */
int vr_debug_model_source_sample(vr_context *ctx, const uint64_t *idx, uint32_t n, uint32_t seed, float *org, float *dir,
                                 uint32_t *draws);
/* ... of the surface source (vr_set_surface_source; gpu/raygSource.hpp:65-81), by the device function its generator
 * runs: origin, direction, start weight and the engine outputs consumed (2) of global ray indices idx[]    */
int vr_debug_surface_source_sample(vr_context *ctx, const uint64_t *idx, uint32_t n, uint32_t seed, float *org, float *dir,
                                   float *weight, uint32_t *draws);
/* ... of the source model in force (vr_set_source_model), by the device function its generator runs: origin, direction,
 * start weight (1 without kHasWeight) and the engine outputs consumed of global ray indices idx[], kernel seed `seed`  */
int vr_debug_user_source_sample(vr_context *ctx, const uint64_t *idx, uint32_t n, uint32_t seed, float *org, float *dir,
                                float *weight, uint32_t *draws);
/* first `count` raw mt19937_64 outputs of the per-ray engine of ray idx      */
int vr_debug_rng_outputs(vr_context *ctx, uint64_t idx, uint32_t seed,
                         uint32_t count, uint64_t *out);
/* unit normals (ntris x 3) and areas (ntris) of the triangle mesh in force, as vr_set_triangles computed them or as
 * vr_set_triangles_device left them on the device (downloaded on demand)     */
int vr_debug_triangle_mesh(vr_context *ctx, float *normals3, float *areas, uint32_t ntris);
/* BVH statistics: nodes, leaves, max depth */
int vr_debug_bvh_stats(vr_context *ctx, uint32_t *out3);
/* consistency of the resident device-built BVH: number of internal nodes whose box is not
 * exactly the union of their children's or whose subtree size is inconsistent (expected 0)  */
int vr_debug_bvh_check(vr_context *ctx, uint32_t *violations);

/* Measurement aid (bench.py's roofline): the instruction-issue ceiling of the device for one of
 * the instruction mixes the hot kernels are made of (0 f32 VALU independent, 1 f32 VALU dependent
 * chain, 2 mt19937_64 seeding steps, 3 SALU, 4 packet-traversal VALU+SALU mix,
 * 5 independent VALU+SALU mix, 7 the absorbing flat-scene tracer's 1.6 : 1 VALU+SALU mix), at `wavesPerSimd`
 * resident waves per SIMD.  out4 = {counted instructions / s, sustained clock Hz, seconds, count} */
int vr_debug_issue_rate(vr_context *ctx, int kind, int wavesPerSimd, uint32_t iters, double *out4);

#ifdef __cplusplus
}
#endif
#endif /* VIENNARAY_AMD_H */
