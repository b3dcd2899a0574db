// vr_context.hpp — private to the translation units of the C ABI (vr_api.cpp names them): the context behind
// include/viennaray_amd.h, the types its fields are made of, and the few functions more than one of those files uses.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdint>
#include <map>
#include <optional>
#include <string>
#include <vector>

#include "../../include/viennaray_amd.h"
#include "vr_host.hpp"
#include "vr_kernels.hpp"
#include "vr_source.hpp"
#include "vr_types.hpp"
#include "vr_bin_grid.hpp"

namespace vr {

template <class T> struct DevBuf {
  T *p = nullptr;
  size_t cap = 0;
  bool holds(size_t n) const { return p && n <= cap; } // (ensure(n) leaves the buffer where it is)
  hipError_t ensure(size_t n) {
    if (holds(n))
      return hipSuccess;
    if (p)
      (void)hipFree(p);
    p = nullptr;
    cap = 0;
    hipError_t e = hipMalloc((void **)&p, std::max<size_t>(n, 1) * sizeof(T));
    if (e == hipSuccess)
      cap = std::max<size_t>(n, 1);
    return e;
  }
  // buffers whose size follows the ray count of an apply(): grown by half again, so a simulation whose
  // ray count creeps up from step to step re-allocates O(log) times, not every step (hipMalloc of a
  // multi-GB ray stream costs tens of ms)
  hipError_t ensure_grow(size_t n) {
    if (holds(n))
      return hipSuccess;
    const size_t want = std::max(n, cap + cap / 2);
    hipError_t e = ensure(want);
    if (e != hipSuccess && want > n) { // (no room for the head-room: the exact size)
      (void)hipGetLastError();
      e = ensure(n);
    }
    return e;
  }
  // ensure(n), then n elements up from the host
  hipError_t upload(const T *src, size_t n) {
    const hipError_t e = ensure(n);
    return e != hipSuccess ? e : hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice);
  }
  // n elements down to the host
  hipError_t download(T *dst, size_t n) const { return hipMemcpy(dst, p, n * sizeof(T), hipMemcpyDeviceToHost); }
  void release() {
    if (p)
      (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) {
    o.p = nullptr;
    o.cap = 0;
  }
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) {
      release();
      std::swap(p, o.p);
      std::swap(cap, o.cap);
    }
    return *this;
  }
  ~DevBuf() { release(); } // (vr_destroy selects the device before the context goes away)
};

// vr_map_to_points*: from this many query points on they are walked in Morton order (DESIGN.md 8n has the measurement)
constexpr uint32_t VR_MAP_SORT_MIN = 1u << 19;
// vr_cast_rays*: from this many rays on they are walked in the Morton order of their origins.  Never, by default: measured
// (profiles/cast_rays_bench.json), the sort shortens the walk of scattered rays but costs more than it saves
// at every ray count up to 10^7 on both scenes of the measurement
constexpr uint32_t VR_CAST_SORT_MIN = 0xFFFFFFFFu;

// Every tuning and experiment switch of the library, read from the environment in ONE place (read_knobs): an apply
// reads them once, at vr_apply_prepare, into vr_context::knobs.  Unless its line says RESULTS, a switch only moves work
// around: the flux and the TraceInfo counters stay bit-exact (tests/test_gpu_parity.py).  (VR_CSRC_DIR / VR_HIPCC /
// VR_CACHE_DIR are configuration of vr_register_particle_model, read there.)
struct Knobs {
  // scene build
  std::optional<uint32_t> accReplicas; // VR_ACC_REPLICAS: flux accumulator replicas, >= 1, rounded down to a power of two (unset: by scene size)
  bool hostBuild = false;              // VR_HOST_BUILD (non-zero): LBVH, neighbourhood and disk areas on the host (validation path)
  std::optional<uint32_t> leafMax;     // VR_LEAF_MAX [1, 15]: primitives per BVH leaf (unset: VR_LEAF_MAX disks, 3 triangles)
  bool noChildOrder = false;           // VR_NO_CHILD_ORDER (non-zero): BVH children not ordered source side first
  float mortonAniso = VR_MORTON_ANISO; // VR_MORTON_ANISO >= 1: largest aspect ratio of the Morton grid's cells
  bool nbTwoPass = false;              // VR_NB_TWO_PASS (set): the neighbourhood query in two passes (count, fill)
  // kernel choice
  bool smallScene = true;              // VR_SMALL_SCENE (0: off): small scenes resident in LDS (MODE 4)
  bool noRelief = false;               // VR_NO_RELIEF (set): no relief packets (MODE 5 / 6) on flat scenes with relief
  float reliefMaxThick = 8.f;          // VR_RELIEF_MAX_THICK: thickest scene (grid cells along the source axis) for relief packets
  float reliefTravel = 1.5f;           // VR_RELIEF_TRAVEL >= 0.05: a ray is loose when thickness x tan(theta) exceeds this (grid cells)
  float reliefTile = 1.f;              // VR_RELIEF_TILE >= 0.25: fine relief tile side in grid cells
  std::optional<int> reliefCoarseK;    // VR_RELIEF_COARSE_K >= 1: fine tiles per coarse tile side (unset: by field size)
  float reliefShare = 0.3f;            // VR_RELIEF_SHARE: largest predicted share of loose rays for relief packets
  float reliefSteps = 6.f;             // VR_RELIEF_STEPS >= 1: a ray crossing more tiles through the scene box is loose
  int reliefLookups = 1;               // VR_RELIEF_LOOKUPS [0, 2]: coarse look-ups of the generator's hit prediction
  bool noSpill = false;                // VR_NO_SPILL (set): the tight general relief kernel keeps its continuing rays
  std::optional<bool> generalFlat;     // VR_GENERAL_FLAT (set): packet-query crediting in the general kernel on (non-zero) / off
  std::optional<bool> absorbCarry;     // VR_ABSORB_CARRY (set): absorbing kernel with (non-zero) / without straggler carry-over
  std::optional<int> traceBlocks;      // VR_TRACE_BLOCKS >= 1: blocks per CU of the trace launch (unset: by occupancy and rays)
  std::optional<int> looseBlocks;      // VR_LOOSE_BLOCKS >= 1: ... of a relief scene's loose launch
  // ray stream
  std::optional<uint64_t> batchRays;   // VR_BATCH_RAYS >= 256: rays per batch (unset: 2^27)
  uint32_t binCap = VR_BIN_CAP;        // VR_BIN_CAP >= 8: record slots per sort bin
  uint32_t raysPerBin = 40;            // VR_RAYS_PER_BIN >= 1: rays per sort bin the grid is sized for
  bool binAlign = true;                // VR_BIN_ALIGN (0: off): sort bins aligned with the disk lattice (3-D, disks; vr_bin_grid.hpp)
  bool uniformDisks = true;            // VR_UNIFORM_DISKS (0: off): the absorbing flat-scene kernel's uniform-disk variants where the scene allows them
  bool planarDisks = true;             // VR_PLANAR_DISKS (0: off): ... the planar one of them (off: planar disks run the uniform-disk kernel)
  bool planarRound = true;             // VR_PLANAR_ROUND (0: off): ... in its one-point-per-round form (off: the planar kernel as it was)
  bool planarLattice = true;           // VR_PLANAR_LATTICE (0: off): ... with its candidates from the lattice table where the cloud is a lattice cloud (off: the one-point-per-round kernel as it was)
  bool latticeLaneTests = true;        // VR_LATTICE_LANE_TESTS (0: off): ... each lane testing the four disks at the corners of its point's cell where the disks are small against the pitch (off: MODE_ABSORB_FLAT_LATTICE as it was)
  bool tileBuckets = true;             // VR_TILE_BUCKETS (0: off): a lattice-lanes launch files its simple rays by lattice tile and finishes them against the tile in LDS (vr_tile_buckets.hpp; off: generator and kernel as they were)
  int tileShift = 6;                   // VR_TILE_SHIFT [1, 6]: ... a tile is 2^shift x 2^shift lattice cells
  std::optional<uint32_t> tileCap;     // VR_TILE_CAP >= 1: ... record slots per bucket (unset: lattice_tile_capacity)
  std::optional<uint32_t> spanBins;    // VR_SPAN_BINS [1, 64]: sort bins per work-queue grab (unset: by trace mode)
  std::optional<uint32_t> numQueues;   // VR_QUEUES (set): >= VR_QUEUES one queue per XCD, else one (unset: by scene)
  // kernel parameters (TraceParams)
  uint32_t pqFrontier = 12;            // VR_PQ_FRONTIER [1, 24]: packet query gives up beyond this frontier
  uint32_t pqCand = 24;                // VR_PQ_CAND [1, 24]: ... or beyond this many candidates
  float pqMargin = 1.5f;               // VR_PQ_MARGIN >= 0: packet query's frontier-cache margin (units of 2 r / 1.7 cells)
  std::optional<float> keyCoord;       // VR_KEY_COORD: sort plane of the ray stream (unset: host_sort_plane)
  uint32_t packetBudget = 128;         // VR_PACKET_BUDGET >= 0: node visits of a packet traversal
  std::optional<uint32_t> walkPark;    // VR_WALK_PARK [1, 100]: % of parked lanes that tests the leaves (unset: 25 disks, 10 triangles)
  uint32_t walkExit = 16;              // VR_WALK_EXIT [1, 64]: a round's walk ends below this many walking lanes
  uint32_t packetRatio = 3;            // VR_PACKET_RATIO >= 1: packet traversal gives up beyond ratio x mean path
  uint32_t debugFlags = 0;             // VR_DEBUG_FLAGS: kernel experiment bits; many of them change RESULTS
  bool noHeightField = false;          // VR_NO_HEIGHT_FIELD (set): no height field over the source plane
  float hfTile = 4.f;                  // VR_HF_TILE >= 0.25: height-field tile side in grid cells
  // results
  uint32_t mapSortMin = VR_MAP_SORT_MIN; // VR_MAP_SORT_MIN: vr_map_to_points* sorts its queries by Morton key from this many on (0: always, 4294967295: never; read at every call, like VR_HOST_SMOOTH); same bits either way
  uint32_t castSortMin = VR_CAST_SORT_MIN; // VR_CAST_SORT_MIN: vr_cast_rays* sorts its rays by the Morton key of their origins from this many on (0: always, 4294967295: never, the default; read at every call); same bits either way
  // diagnostics
  bool printLaunches = false;          // VR_PRINT_LAUNCHES (set): trace-launch times and spilled rays on stderr
  bool hostSmooth = false;             // VR_HOST_SMOOTH (set): vr_smooth_flux on the host
  bool debugWalk = true;               // VR_DEBUG_WALK (0: the escape-link walk): vr_debug_intersect's walk
  bool logPlainAtomics = false;        // VR_LOG_PLAIN_ATOMICS (set): the data log without its per-block LDS copy (A/B of DESIGN.md 8c)
#ifdef VR_DIAG
  bool skipTight = false;              // VR_SKIP_TIGHT (set): a relief scene's loose launch alone; INCOMPLETE results
  bool skipLoose = false;              // VR_SKIP_LOOSE (set): ... its tight launch alone; INCOMPLETE results
#endif
};

// one entry of vr_set_particles (a deep copy of the caller's vr_particle)
struct ParticleSpec {
  int kind = 0;
  float sticking = 1.f, sourcePower = 1.f, coneAngle = 0.f, meanFreePath = -1.f;
  float params[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int userModel = -1;   // kind >= VR_PARTICLE_USER_BASE: index of the run-time model
  int kernelKind = 0;   // the kind its kernel sees: inside its own code object a run-time model is the registry's last entry
  uint32_t numData = 1; // its data labels
  std::vector<int32_t> matIds;
  std::vector<float> matVals;
};
// a particle model registered at run time (vr_register_particle_model): its own code object with the extended trace
// kernels, the model compiled in as entry VR_BUILTIN_MODELS of that module's registry
struct UserModel {
  std::string name;
  hipModule_t module = nullptr;
  int numData = 1;
  bool needsFull = false;
  int numState = 0;                     // kStateWords of a stateful model (0: stateless)
  int logRows = 0;                      // kLogRows: rows of the data log its log_data hook writes (0: no hook)
  std::map<int, hipFunction_t> kernels; // key: module_kernel_key(D, geo, mode), vr_types.hpp
  hipFunction_t gen[2] = {nullptr, nullptr}; // a stateful model's generator (gen_state_kernel), 2-D / 3-D
  // flux statistics: the module's twin with the statistics compiled in (VR_USER_FLUX_STATS), built from the kept text
  // when a statistics-on apply first needs it, under a cache key of its own
  std::string source;
  hipModule_t statsModule = nullptr;
  std::map<int, hipFunction_t> statsKernels; // key as `kernels`
};
// a source model registered at run time (vr_register_source_model): its own code object with the generator
// (gen_user_source_kernel) and its debug twin, no trace kernel
struct SourceModel {
  std::string name;
  std::string codeObject;                                         // path of the cached code object: the text's identity
  hipModule_t module = nullptr;
  bool hasWeight = false;                                         // VrUserSource::kHasWeight
  hipFunction_t gen[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}}; // [2-D / 3-D][records without / with the RNG cursors]
  hipFunction_t debug[2] = {nullptr, nullptr};                    // debug_user_source_kernel, 2-D / 3-D
};

// The prepared launch of one particle of an apply() (vr_context::launches: one per particle of vr_set_particles).
// params holds everything but the buffers all particles share — ray stream, scratch, counters, accumulators — whose
// addresses launch_params adds when the launch runs.
struct ParticleLaunch {
  TraceParams params{};
  uint32_t slot = 0;     // index of the particle: its counter block, wall-table / frame slot
  uint32_t dataBase = 0; // its first accumulator plane
  bool stats = false;    // flux statistics: two companion planes behind its data labels (planes numData, numData + 1)
  unsigned grid = 0;
  int traceMode = MODE_GENERAL, kernelParticle = 0;
  // the mode launch_trace takes: traceMode, except on the ladder of the absorbing flat-scene kernel's variants, where a
  // MODE_ABSORB_FLAT launch runs the highest of modes 8 to 12 that the scene, the knobs and the catalogue allow
  // (vr_prepare.cpp: absorb_flat_kernel_mode).  mode_traits(kernelMode) says which frame words the launch carries:
  // uniform VR_F_UD_*, planar VR_F_PD_*, planarRound VR_F_PR_*, lattice VR_F_PL_*
  int kernelMode = MODE_GENERAL;
  bool latticeLanesScene = false; // (lattice_lanes_rule's verdict on the scene alone, for the VR_PRINT_LAUNCHES line)
  // The tile buckets of a lattice-lanes launch (vr_prepare.cpp: plan_tile_buckets; vr_tile_buckets.hpp): the launch's
  // simple rays go through gen_tile_kernel and tile_trace_kernel, the others through the record stream's overflow region and kernelMode's kernel
  // as before.  tile: everything but the batch's own fields (tileCount, slotBase, tileCap: run_batch)
  bool tileBuckets = false;
  TileParams tile{};
  double tileSide = 0., tileSrcArea = 0.; // a tile's side and the source rectangle's area: lattice_tile_capacity's operands
  bool absorb = false;
  bool recExtra = false; // the records' side array (TraceParams::recExtra)
  hipFunction_t userKernel = nullptr; // the trace kernel of a run-time model (nullptr: a kernel of the library)
  Generator gen = GEN_RANDOM;         // the generator of the launch, by the source in force (fill_trace_params)
  hipFunction_t userGen = nullptr;    // a module's generator that runs instead: a stateful model's (init, then the sample of
                                      // `gen`), or the source model's where gen == GEN_SOURCE_MODEL (nullptr: the library's `gen`)
  bool genWeights = false;            // the generator writes the batch's start weights (surface source, source model with kHasWeight)
  SourceCtx source{};                 // what the source model sees of this launch
  DevBuf<float> primSticking;         // this particle's per-primitive sticking, leaf order (params.primSticking, or unused)
  DevBuf<int32_t> matTable;           // its (id, value) table for launch_prim_sticking: the ids, then the values' bits
  std::vector<int32_t> matTableHost;  // (staging of that upload)
  bool relief = false; // flat with relief: a second launch (looseMode, looseGrid) traces the loose bins
  bool binAlign = false; // the sort bins follow the disk lattice where size_bins can make them (VR_BIN_ALIGN)
  BinGrid binGrid;       // the sort-bin grid of a full batch (VR_PRINT_LAUNCHES)
  int looseMode = MODE_GENERAL;
  unsigned looseGrid = 0;
  vr_trace_info info{};
};

} // namespace vr

using namespace vr; // (struct vr_context is declared at global scope by the public header)

struct vr_context {
  int device = 0;
  int numCUs = 256;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::string err;

  HostGeometry geo;          // the scene's description, and the host mirror of its arrays (vr_host.hpp says which is which)
  bool geoOnDevice = false;  // a device setter filled the resident buffers itself: build_scene uploads nothing
  bool hostGeoValid = false; // ... and ensure_host_geometry has downloaded the mirror since
  bool geometryDirty = true; // BVH / uploads need rebuilding
  bool configDirty = true;   // bbox / walls / areas / sticking map need recomputing
  Bvh bvh;
  std::vector<uint32_t> leafOfOrig;
  std::vector<float> diskAreas;       // host mirror of dAreas (disks), downloaded on demand
  bool diskAreasHostValid = false;

  // Trace<T,D> configuration (rayTrace.hpp:157-179, rayUtil.hpp:83-94)
  int bcs[3] = {0, 0, 0};
  int sourceDirection = -1; // -1: default by D (POS_Y for 2-D, POS_Z for 3-D)
  bool usePrimaryDirection = false;
  float primaryDirection[3] = {0, 0, 0};
  bool useWdist = false;
  uint32_t totalData = 1;         // data labels of all particles of the apply: accumulator planes, TracingData vectors
  uint32_t accPlanes = 0;         // planes the accumulator buffers currently hold
  // flux statistics (vr_set_flux_statistics): every particle of the apply keeps VR_STAT_PLANES companion planes behind
  // its data labels — the sum of squares and the hit count of label 0 — in the same array, so gather, overflow check,
  // bound buffers and the sharded all-reduce see them like any other plane
  bool fluxStats = false;
  uint32_t totalPlanes() const { return totalData + (fluxStats ? (uint32_t)VR_STAT_PLANES * (uint32_t)numParticles() : 0u); }
  // the plane of data label `dataIdx` (counted over all particles, as vr_get_flux_data counts them)
  uint32_t planeOfData(uint32_t dataIdx) const {
    if (!fluxStats)
      return dataIdx;
    uint32_t base = 0;
    for (size_t q = 0; q < specs.size(); ++q) {
      if (dataIdx < base + specs[q].numData)
        return dataIdx + (uint32_t)VR_STAT_PLANES * (uint32_t)q;
      base += specs[q].numData;
    }
    return dataIdx;
  }
  // the first plane of particle q
  uint32_t planeBase(uint32_t q) const {
    uint32_t base = 0;
    for (size_t k = 0; k < q && k < specs.size(); ++k)
      base += specs[k].numData + (fluxStats ? (uint32_t)VR_STAT_PLANES : 0u);
    return base;
  }
  DevBuf<float> dRayState;            // a stateful model's per-ray state of one batch (the frame's VR_F_STATE_*), float4 per ray
  DevBuf<int32_t> dPrimMaterial;      // material id per original primitive for a stateful model (VR_F_MAT_*)
  // the material ids on the device, caller's order: what prepare_sticking and the stateful models read.  Set from the
  // device (materialOnDevice: materialIds is then a mirror nobody fills) or uploaded from materialIds when stale.
  std::vector<int32_t> materialIds;
  DevBuf<int32_t> dMaterialIds;
  uint32_t materialCount = 0;         // ids dMaterialIds holds (a primitive beyond them has id 0)
  bool materialOnDevice = false, materialStale = true;
  // the data log (vr_set_data_log_shape): int64 sums of the log_data hooks, rows concatenated, the control words behind
  // them (VR_LOG_*, vr_frame.hpp); zeroed at every launch, summed over the batches and particles of an apply on the device
  std::vector<uint32_t> logRowSizes;
  uint32_t logTotal = 0;              // entries of all rows
  bool logActive = false;             // the prepared apply fills the log (a shape is set)
  DevBuf<unsigned long long> dDataLog;
  std::vector<unsigned long long> logCtlHost; // staging of the control words' upload
  std::vector<unsigned long long> logHost;    // the last apply's sums + [dropped] (vr_get_data_log*)
  bool haveLog = false;
  std::vector<UserModel> userModels;
  bool particleDirty = true;      // vr_set_particles: the sticking map needs recomputing
  std::vector<ParticleSpec> specs;      // vr_set_particles (empty: none set yet): > 1 entries = a multi-particle apply
  size_t numParticles() const { return std::max<size_t>(1, specs.size()); } // (what the per-particle buffers are sized for)
  std::vector<ParticleLaunch> launches; // prepared by vr_apply_prepare: one per particle (at least one)
  Knobs knobs;                          // the tuning switches, read by vr_apply_prepare
  // Trace::setGlobalData: vectors (padded to one stride) and scalars, resident in HBM
  std::vector<std::vector<float>> globalVecs;
  std::vector<float> globalScalars;
  bool globalDirty = false;
  uint32_t globalStride = 0;
  DevBuf<float> dGlobalVec, dGlobalScalars;
  // A vector set from device memory (vr_set_global_data_device) is written into its row of dGlobalVec when it is set:
  // globalVecs[v] is then only a mirror, left empty as long as no host path asks for the values (none does today).
  // Per vector: its length, whether the row on the device is the truth, whether a host-set vector still has to go up.
  struct GlobalRow {
    uint32_t len = 0;
    bool onDevice = false, pending = false;
  };
  std::vector<GlobalRow> globalRows; // (one per entry of globalVecs)
  uint32_t globalRowsLaid = 0;       // rows of dGlobalVec, at globalStride, that hold what they should
  bool anyGlobalOnDevice() const {
    for (const GlobalRow &r : globalRows)
      if (r.onDevice)
        return true;
    return false;
  }
  // the ray source in force (vr_source.hpp) and the device buffers of the sources, which are kept across switches
  RaySource src;
  float sourceAreaOverride = 0.f;  // Source::getSourceArea() of a user source (<= 0: SourceRandom's, the bbox face)
  DevBuf<float> dSurfPos, dSurfNrm, dSurfWeights;       // a surface source's tables, uploaded when they are set
  DevBuf<float> dSurfPosIn, dSurfNrmIn, dSurfWeightsIn; // vr_set_surface_source_device packs into these; accepted: swapped in
  DevBuf<unsigned long long> dSurfBad;                  // ... and its one word of validation
  DevBuf<float> dSurfRayWeights;   // start weight of every ray of one batch (TraceParams::hostWeights where the generator writes them)
  std::vector<SourceModel> sourceModels; // vr_register_source_model
  DevBuf<float> dSrcTable;         // the table of the source model in force
  DevBuf<float> dGrid, dHostOrg, dHostDir, dHostWeights; // a grid's / the host rays' arrays, uploaded at prepare (upload_source_data)
  DevBuf<uint32_t> dHostDraws;
  uint64_t reserveRays = 0;        // vr_reserve_rays: the ray-stream buffers hold at least this many rays
  uint64_t numRaysPerPoint = 1000, numRaysFixed = 0;
  uint32_t maxReflections = 0xFFFFFFFFu, maxBoundaryHits = 1000;
  uint32_t rngSeed = 0;
  bool useRandomSeed = true;
  uint32_t runNumber = 1;
  uint64_t rayFirst = 0, rayCount = 0;
  bool haveSharedSeed = false; // vr_apply_sharded + useRandomSeed: rank 0's draw, handed round by the all-reduce;
                               // a multi-particle apply with random seeds: its one draw
  bool keepSharedSeed = false; // (the sharded entry point clears the seed itself)
  size_t numGenLaunches = 0, numTraceLaunches = 0;
  uint32_t sharedSeed = 0;

  // derived at prepare()
  float bbLo[3], bbHi[3];
  std::array<int, 5> ts{};
  int boundaryConds[2] = {0, 0};
  float sourceArea = 0.f;
  uint64_t numRaysLast = 0;
  bool prepared = false, launched = false, haveResult = false;

  vr_trace_info info{};
  double buildSeconds = 0.0;

  // device buffers
  DevBuf<float> dNodes, dPrims;
  DevBuf<float> dAreas, dFluxTmp;     // exposed area per primitive (caller's order); normalisation scratch
  DevBuf<uint32_t> dNormMax;          // flux_max_kernel's reduction word
  // vr_map_to_points*: the query sort's pairs and tables, the flux variant's per-primitive values, the host form's
  // staging (values, points, normals, out) and, in a VR_DIAG build, the node-visit counter.  Grown behind host_waits only
  DevBuf<unsigned long long> dMapKeysA, dMapKeysB, dMapVisits;
  DevBuf<uint32_t> dMapValsA, dMapValsB, dMapSortTable, dMapScanTmp;
  DevBuf<float> dMapFlux, dMapValues, dMapPoints, dMapNormals, dMapOut;
  // vr_cast_rays*: the launch parameters the last prepare_one left (pair nodes, records, wall table and boundary codes of
  // its launch frame; the shared buffers' addresses are taken when a cast runs), good while castValid and castBuild is the
  // build count; the walk's overflow word of a cast (its own: an apply's counters are not touched); the host form's staging.
  // The ray sort shares the map's pairs and tables above: both run on the context's stream, one after the other
  TraceParams castParams{};
  bool castValid = false;
  uint32_t castBuild = 0;
  DevBuf<unsigned long long> dCastCounters;
  DevBuf<float> dCastOrg, dCastDir, dCastDist, dCastHit;
  DevBuf<int32_t> dCastPrim;
  DevBuf<uint32_t> dCastBh;
  // vr_gather_flux*: the int64 sums of one call's range, and the host form's staging (out, emission; the debug entry
  // point's rows too).  They read castParams like a cast and share its counter block.  Grown behind host_waits only
  DevBuf<unsigned long long> dGatherAcc;
  DevBuf<float> dGatherOut, dGatherEmission;
  // vr_gather_paths*: the reflectivity table in leaf order, its verdict word, and the host form's staging of the table;
  // the sums and the output staging are the gather's.  Grown behind host_waits only
  DevBuf<float> dPathRho, dPathIn;
  DevBuf<uint32_t> dPathWord;
  // vr_gather_sums* / vr_gather_adaptive*: the int64 sums of the squared weights beside dGatherAcc, the two primitive
  // lists a round reads and writes, the decide kernel's block counts with the word that comes back behind them, and the
  // host forms' staging of stdErr and samplesUsed.  Grown behind host_waits only.  vr_gather_species_adaptive* keeps
  // numSpecies of each sum and output, a list's masks behind the list (2 primCount words) and five words per round
  DevBuf<unsigned long long> dGatherAccSq;
  DevBuf<uint32_t> dGatherListA, dGatherListB, dGatherWords, dGatherUsed;
  DevBuf<float> dGatherErr;
  // vr_gather_angular*: the three angular laws of the call in flight, 3 x GATHER_LAW_MAX floats (written by a kernel from
  // its own arguments on c->stream, so behind an earlier call that still reads them).  Grown behind host_waits only
  // vr_gather_species* keeps numSpecies of each in the gather's own buffers: sums, laws, reflectivities, verdict words
  DevBuf<float> dGatherLaws;
  // vr_gather_energy*: the three energy tables of the call in flight beside them, 3 x GATHER_LAW_MAX floats, written and
  // grown the same way
  DevBuf<float> dGatherEnergy;
  // vr_radiosity_*: the link table of the last vr_radiosity_links_device (slots x samples int32 in leaf order,
  // vr_radiosity.hpp), its direct sums and leaf -> original id table, what it was built from, and a solve's work buffers
  // (leaf order: reflectivity, F, the two emission tables; the words that come back; the host forms' staging).  A table
  // is good while radValid and radStamp describes the settings in force (vr_radiosity_solve.cpp: radiosity_stale)
  struct RadiosityStamp {
    uint32_t build = 0, numPrims = 0;
    int bcs[3] = {0, 0, 0}, sourceDirection = -1;
    uint32_t maxBoundaryHits = 0, seed = 0, samples = 0;
    float cosinePower = 0.f;
  };
  bool radValid = false;
  RadiosityStamp radStamp;
  DevBuf<int32_t> dRadLinks, dRadDebug;
  DevBuf<unsigned long long> dRadDirect;
  DevBuf<uint32_t> dRadOrigOfLeaf, dRadWords;
  DevBuf<float> dRadRho, dRadF, dRadE0, dRadE1, dRadIn, dRadOut;
  bool areasValid = false;
  DevBuf<uint32_t> dNbOff, dNbIds, dLeafOfOrig;
  DevBuf<uint32_t> dNbTmp; // the one-pass neighbourhood query's fixed-stride lists (build scratch)
  uint32_t nbTotal = 0;               // entries of the resident neighbourhood CSR
  DevBuf<unsigned long long> dFluxAcc, dFluxOrig, dCounters, dScratch;
  DevBuf<unsigned long long> dWorkQ;  // span cursors of the trace kernel's per-XCD queues
  size_t scratchWaves = 0;
  // flux accumulators are replicated accReplicas times (power of two, stride accStride
  // elements); a block credits replica blockIdx & (accReplicas-1): small scenes would
  // otherwise serialise every credit of the chip on a handful of cache lines
  uint32_t accReplicas = 1, accStride = 0;
  // device-side setup (vr_ingest.hip, vr_bvh.hip, vr_sort.hip)
  DevBuf<float> dDisk4, dNormal3, dPoints3, dVerts, dBox, dSBox, dNodeBox;
  DevBuf<float> dTriAreas;                // a device-set mesh's areas, written by launch_pack_mesh only (compute_areas copies them into dAreas)
  DevBuf<unsigned long long> dIngestKeys; // launch_ingest_disks' / launch_scan_mesh's block partials
  DevBuf<float> dIngestBounds;            // ... their six bounds, and launch_scan_mesh's word behind them
  DevBuf<double> dSortPlane;              // launch_sort_plane's block partials, then the 512 merged sums
  hipEvent_t evIn = nullptr, evOut = nullptr; // hand-over between a caller's stream and this context's (device entry points)
  DevBuf<uint32_t> dTris, dBounds, dValsA, dValsB, dSortTable, dRangeLo, dRangeHi, dChildL, dChildR, dParentInt,
      dParentLeaf, dArrive, dOrder, dSubSize, dQNodes, dPNodes, dWalkStack;
  size_t walkStackWaves = 0;
  DevBuf<float> dNodesPre, dWide;
  uint32_t wideRoot[3] = {0, 0, 0};  // 64-ary tree: root's first child, count | flag, primitive base
  bool haveWide = false;
  float sceneLo[3] = {0, 0, 0}, sceneHi[3] = {0, 0, 0};
  uint32_t numNodes = 0;         // traversal nodes emitted by the builder
  float qbase[3] = {0, 0, 0}, qscale[3] = {0, 0, 0}; // frame of the 16-byte nodes
  float keyCoord = 0.f;          // sort plane of the ray stream on the tracing axis (host_sort_plane)
  float keyShare = 1.f;          // share of the surface shown to the source that lies in that plane
  // uniform disks (build_scene, once per geometry commit: launch_uniform_disks over the packed records): every disk has
  // record 0's normal and radius, word for word.  false for a mesh and for an empty scene.
  bool uniformDisks = false;
  uint32_t uniformWords[4] = {0, 0, 0, 0}; // ... those words: n.x, n.y, n.z, radius
  // ... and planar (vr_planar_disks.hpp): that normal is +-1 along planarAxis and +-0 along the two others, every centre
  // carries planarWord in that coordinate, every centre coordinate is finite
  bool planarDisks = false;
  int planarAxis = 0;
  uint32_t planarWord = 0;
  DevBuf<uint32_t> dUniformDisks;          // launch_uniform_disks' VR_UNIFORM_WORDS words
  // ... and a lattice cloud (vr_planar_lattice.hpp; build_scene, behind the BVH's leaf order): dLattice holds the table
  // uint32[latticeN[1]][latticeN[0]] of leaf positions, and behind it launch_lattice_table's flag word.  The phases are the
  // smallest centre coordinates along the plane's two in-plane axes, the pitch is the scene's gridDelta
  bool planarLattice = false;
  int latticeN[2] = {0, 0};
  float latticePhase[2] = {0.f, 0.f};
  DevBuf<uint32_t> dLattice;
  SetupParams lastSetup{};       // buffers of the resident device build (vr_debug_bvh_check)
  bool haveSetup = false;
  int builtOrderAxis = -1;       // child order of the resident BVH (source side first)
  int bvhRefits = 0;             // 1 if the last build had to be re-fitted with agent-scope fences
  uint32_t bvhBuilds = 0;        // scene builds of this context
  float builtOrderSign = 0.f;
  DevBuf<unsigned long long> dKeysA, dKeysB;
  bool hostOrderValid = false;   // c->bvh.order mirrors dOrder
  bool hostNeighborsValid = false;
  // ray stream (one batch)
  DevBuf<float> dSlotRec, dWalls;
  DevBuf<uint32_t> dBinCount;
  DevBuf<uint32_t> dTileCount; // tile buckets: VR_TILE_MAX_TILES cursors (TileParams::tileCount)
  int tileGenBlocks = 0;       // ... resident blocks per CU of the tile generator on this context's device (0: not asked yet)
  int tileLdsShift = 0;        // ... the largest tile size the tile kernel's dynamic LDS was allowed for on it (0: the default limit)
  size_t slotStride = 0; // record slots of the ray-stream buffer (bins + overflow region)
  uint32_t raysPerBin = 40;
  DevBuf<uint32_t> dScanTmp;
  uint32_t batchCap = 0;      // rays per batch the buffers hold
  uint32_t numBins = 0;
  uint64_t rayFirstLaunch = 0, rayEndLaunch = 0;
  float wallsHost[96] = {0};        // the eight wall triangles (made with the bounding box)
  std::vector<float> frameHostAll;  // wall table + scalar frame of every particle of the apply (staging of their uploads)
  // relief field over the source plane (ReliefParams): scenes that are flat with relief
  DevBuf<uint32_t> dRfRawLo, dRfRawHi, dRfStats;
  DevBuf<float> dRfFine, dRfCoarse;
  ReliefParams rf{};
  uint32_t rfBuild = 0xFFFFFFFFu;
  int rfAxes[4] = {-1, -1, -1, -1};
  float rfLooseShare = 1.f;
  DevBuf<float> dSpillRec;     // the general relief kernel's spill queue (TraceParams::spillRec), 16 floats per ray of a batch
  DevBuf<uint32_t> dSpillCount;
  DevBuf<uint32_t> dHfRaw;    // height field over the source plane (HeightFieldParams): built for particles that reflect
  DevBuf<float> dHf;
  HeightFieldParams hf{};
  uint32_t hfBuild = 0xFFFFFFFFu; // the bvhBuilds count and source frame it was made for
  int hfAxes[4] = {-1, -1, -1, -1};
  DevBuf<float> dRecExtra;    // the records' side array (ParticleLaunch::recExtra)
  std::vector<hipEvent_t> evK; // trace-kernel event pairs, one per batch
  std::vector<hipEvent_t> evG; // generator event pairs, one per batch
  double traceKernelSeconds = 0.0;
  uint32_t worldSize = 1;     // ranks whose accumulators will be summed (vr_set_world_size): head-room of the overflow check
  unsigned long long *boundFlux = nullptr; // caller-owned accumulator buffer
  uint32_t boundFluxN = 0;
  unsigned long long *fluxOut() { return boundFlux ? boundFlux : dFluxOrig.p; }
};

#define VR_HIP(ctx, call)                                                                                              \
  do {                                                                                                                 \
    hipError_t e__ = (call);                                                                                           \
    if (e__ != hipSuccess) {                                                                                           \
      (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e__);                                                 \
      return VR_E_HIP;                                                                                                 \
    }                                                                                                                  \
  } while (0)

#define VR_TRY(call)                                                                                                   \
  do {                                                                                                                 \
    const int r__ = (call);                                                                                            \
    if (r__ != VR_OK)                                                                                                  \
      return r__;                                                                                                      \
  } while (0)

namespace vr {

// vr_api.cpp
int fail(vr_context *c, int code, const char *msg);
int hand_over(vr_context *c, std::initializer_list<const void *> buffers, const char *refusal, void *stream);
int host_waits(vr_context *c);
int caller_waits(vr_context *c, void *stream);
// vr_knobs.cpp
Knobs read_knobs();
// vr_models.cpp
int ensure_stats_module(vr_context *c, UserModel &um);
// vr_scene.cpp
int ensure_host_geometry(vr_context *c);
int ensure_host_order(vr_context *c);
int ensure_host_neighbors(vr_context *c);
int build_scene(vr_context *c);
int ensure_device_material_ids(vr_context *c);
int lay_global_rows(vr_context *c, uint32_t rows, uint32_t stride);
// vr_prepare.cpp
BinGrid size_bins(const vr_context *c, bool align, uint64_t count, uint32_t ovCap, TraceParams &p, uint32_t &numBins);
void size_loose(int D, TraceParams &p);
// vr_apply.cpp
const ParticleLaunch &current_launch(const vr_context *c);
TraceParams launch_params(const vr_context *c, const ParticleLaunch &L);

// vr_cast_rays.cpp: what every walk over the resident scene (a cast, a gather) refuses and starts from
int resident_scene_refusal(vr_context *c, const char *api, const char *what);
int resident_scene_params(vr_context *c, bool &waited, TraceParams &p);

// vr_gather_flux.cpp: what a gather refuses and launches with, shared with the link recording (vr_radiosity_solve.cpp)
int gather_refusal(vr_context *c, const char *api, uint32_t primFirst, uint32_t primCount, uint32_t samples, float cosinePower,
                   uint32_t mode, const void *emission, const void *out);
int gather_params(vr_context *c, bool &waited, TraceParams &p, GatherArgs &a, uint32_t primFirst, uint32_t primCount,
                  uint32_t samples, float cosinePower, uint32_t mode);
void gather_cut_chunks(GatherArgs &a, unsigned slabs);
// vr_gather_paths.cpp: what a path gather refuses beyond that, and its reflectivity table into leaf order (c->dPathRho),
// shared with the sums and the adaptive gather (vr_gather_adaptive.cpp)
int paths_refusal(vr_context *c, const char *api, uint32_t primFirst, uint32_t primCount, uint32_t samples, float cosinePower,
                  uint32_t reflection, uint32_t maxBounces, const float *reflectivity, float scalar, const void *out);
int paths_table(vr_context *c, const char *api, const float *rho);
// vr_gather_angular.cpp: the angular laws of a call (laws == nullptr, or all three tables NULL: none).  gather_laws_refusal
// checks them on the host — before anything is touched — against the call's cosinePower, sample budget and dimension and
// leaves them normalised in `set`; gather_laws_args puts them on the device and into the launch arguments
struct GatherLawSet {
  bool any = false;
  uint32_t count[3] = {0, 0, 0};
  float gL = 1.f;
  double wbound = 1.; // (g_L max L or g) max Y: the largest weight a path of the call can have
  float table[3 * 256] = {}; // (GATHER_LAW_MAX each)
};
int gather_laws_refusal(vr_context *c, const char *api, const vr_gather_laws *laws, float cosinePower, uint32_t samples,
                        GatherLawSet &set);
int gather_laws_args(vr_context *c, bool &waited, const GatherLawSet &set, GatherArgs &a);
// vr_gather_energy.cpp: the energy tables of a call (energy == nullptr: none — the call is the angular one).
// gather_energy_refusal checks them on the host, before anything is touched, against the angular call's wbound and the
// sample budget and leaves them in `set`; gather_energy_args puts them on the device and into `ea` (all but ea.a);
// gather_launch is the one place a path gather's samples are launched from: the energy kernel with ea (its .a taken from
// a), the gather's own without
struct GatherEnergySet {
  bool any = false;
  uint32_t count[3] = {0, 0, 0}; // yield, quantiles, retention (vr_gather.hpp: GATHER_ENERGY_*)
  float energyMax = 1.f, sourceEnergy = 0.f;
  uint32_t zeros = 0; // the cut's Z0; 0: no cut
  float table[3 * 256] = {}; // (GATHER_LAW_MAX each)
};
int gather_energy_refusal(vr_context *c, const char *api, const struct vr_gather_energy *energy, double wboundAngular, uint32_t samples,
                          GatherEnergySet &set);
int gather_energy_args(vr_context *c, bool &waited, const GatherEnergySet &set, GatherEnergyArgs &ea);
int gather_launch(vr_context *c, const TraceParams &p, const GatherArgs &a, const GatherEnergyArgs *ea, unsigned slabs);
// the entry points of vr_gather_paths.cpp, vr_gather_adaptive.cpp, vr_gather_angular.cpp and vr_gather_energy.cpp share one
// implementation each (laws == nullptr: the former; energy != nullptr: the latter, whose one-path walk also fills
// energyOut4); `api` names the entry point in the messages
int paths_call_device(vr_context *c, const char *api, const vr_gather_laws *laws, uint32_t primFirst, uint32_t primCount,
                      uint32_t samples, float cosinePower, uint32_t reflection, uint32_t maxBounces, const float *reflectivity,
                      float reflectivityScalar, float *out, void *stream, const struct vr_gather_energy *energy = nullptr);
int paths_call_host(vr_context *c, const char *api, const vr_gather_laws *laws, uint32_t primFirst, uint32_t primCount,
                    uint32_t samples, float cosinePower, uint32_t reflection, uint32_t maxBounces, const float *reflectivity,
                    float reflectivityScalar, float *out, const struct vr_gather_energy *energy = nullptr);
int paths_call_debug(vr_context *c, const char *api, const vr_gather_laws *laws, uint32_t prim, uint32_t sample, float cosinePower,
                     uint32_t reflection, uint32_t maxBounces, const float *reflectivity, float reflectivityScalar,
                     uint32_t maxVertices, uint32_t *vertexIds, float *vertexData, uint32_t *numVertices, uint32_t *end,
                     float *finalDirection3, float *throughput, float *weight, const struct vr_gather_energy *energy = nullptr,
                     float *energyOut4 = nullptr);
int sums_call_device(vr_context *c, const char *api, const vr_gather_spec *spec, const vr_gather_laws *laws, uint32_t primFirst,
                     uint32_t primCount, uint32_t chunkFirst, uint32_t chunks, uint32_t budget, int64_t *sum, int64_t *sumSq,
                     void *stream, const struct vr_gather_energy *energy = nullptr);
int sums_call_host(vr_context *c, const char *api, const vr_gather_spec *spec, const vr_gather_laws *laws, uint32_t primFirst,
                   uint32_t primCount, uint32_t chunkFirst, uint32_t chunks, uint32_t budget, int64_t *sum, int64_t *sumSq,
                   const struct vr_gather_energy *energy = nullptr);
int adaptive_call_device(vr_context *c, const char *api, const vr_gather_spec *spec, const vr_gather_laws *laws, uint32_t primFirst,
                         uint32_t primCount, uint32_t minSamples, uint32_t maxSamples, float relTarget, float absTarget,
                         float *flux, float *stdErr, uint32_t *samplesUsed, vr_gather_adaptive_info *info, void *stream,
                         const struct vr_gather_energy *energy = nullptr);
int adaptive_call_host(vr_context *c, const char *api, const vr_gather_spec *spec, const vr_gather_laws *laws, uint32_t primFirst,
                       uint32_t primCount, uint32_t minSamples, uint32_t maxSamples, float relTarget, float absTarget, float *flux,
                       float *stdErr, uint32_t *samplesUsed, vr_gather_adaptive_info *info,
                       const struct vr_gather_energy *energy = nullptr);

// a work buffer of the map or of a cast grows behind host_waits only (vr_api.cpp: a buffer that moves)
template <class T> int map_grow(vr_context *c, DevBuf<T> &b, size_t n, bool &waited) {
  if (b.holds(n))
    return VR_OK;
  if (!waited) {
    VR_TRY(host_waits(c));
    waited = true;
  }
  VR_HIP(c, b.ensure_grow(n));
  return VR_OK;
}

inline uint64_t rays_of_apply(const vr_context *c) {
  return c->src.rays_of_apply(c->geo.numPrims, c->numRaysPerPoint, c->numRaysFixed);
}

// head-room bits of the overflow checks: the sums of `worldSize` ranks (vr_set_world_size) must still fit a signed int64
inline unsigned rank_headroom(uint32_t worldSize) {
  unsigned bits = 0;
  while ((1u << bits) < worldSize)
    ++bits;
  return bits;
}

} // namespace vr
