// vr_apply.cpp — a prepared apply() on the device: the batches of the ray stream (vr_apply_launch), counters and
// timings back (vr_apply_finish), and the sharded multi-GPU apply.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "vr_context.hpp"
#include "vr_frame.hpp"
#include "vr_lattice_tiles.hpp"

namespace vr {

// The launch the readers of "the" prepared launch see (vr_get_trace_mode, the vr_debug_* entry points, the spill print
// of VR_PRINT_LAUNCHES): the LAST one prepared — after a multi-particle prepare, the last particle's.
const ParticleLaunch &current_launch(const vr_context *c) { return c->launches.back(); }

static hipEvent_t &event_at(std::vector<hipEvent_t> &v, size_t i, vr_context *c, int &rc) {
  while (v.size() <= i) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) {
      rc = fail(c, VR_E_HIP, "hipEventCreate failed");
      static hipEvent_t none = nullptr;
      return none;
    }
    v.push_back(e);
  }
  return v[i];
}

// A prepared launch's parameters with the addresses of the buffers every particle of the apply shares (ray stream,
// scratch, work queues, counter blocks, accumulator planes) as they are now: a later particle's prepare may have grown one.
TraceParams launch_params(const vr_context *c, const ParticleLaunch &L) {
  TraceParams p = L.params;
  p.slotRec = c->dSlotRec.p;
  p.binCount = c->dBinCount.p;
  p.walkStack = c->dWalkStack.p;
  p.rngScratch = c->dScratch.p;
  p.workCounter = c->dWorkQ.p;
  p.recExtra = L.recExtra ? c->dRecExtra.p : nullptr;
  const bool spill = L.relief && L.looseMode == MODE_RESUME;
  p.spillRec = spill ? c->dSpillRec.p : nullptr;
  p.spillCount = spill ? c->dSpillCount.p : nullptr;
  p.counters = c->dCounters.p + C_BLOCK * (size_t)L.slot;
  p.fluxAcc = c->dFluxAcc.p + (size_t)L.dataBase * p.planeStride; // (this particle's planes)
  return p;
}

// Tile buckets: the rays of a batch that the lattice-lanes kernel is expected to trace at most — those that cross a wall or
// fall through a hole, an eighth of the batch — for the sizes of its grid and of its queue's spans (more of them are traced
// all the same: the grid is persistent, the spans only deal the work out)
static uint32_t tile_bin_rays(uint32_t count) { return (uint32_t)std::min<uint64_t>(count, std::max<uint64_t>(4096, count / 8)); }

// the batch's own fields of a particle's launch parameters: sort bins, spans per queue grab, queues
// tiles: a tile-bucket launch (vr_tile_buckets.hpp) — no sort bins, the rays its tile kernel does not finish lie in the
// overflow region; binRays: how many of them the queue's spans and the grid are sized for
static TraceParams batch_params(vr_context *c, const ParticleLaunch &L, uint64_t first, uint32_t count, bool tiles = false) {
  const uint32_t binRays = tiles ? tile_bin_rays(count) : count;
  const Knobs &K = c->knobs;
  TraceParams p = launch_params(c, L);
  p.batchFirst = first;
  p.batchCount = count;
  // (the grid of THIS launch's full batch, L.params: the particles of a list differ in it where one has relief packets)
  const TraceParams &s = L.params;
  uint32_t nbBatch = s.numBins;
  size_bins(c, L.binAlign, count, c->batchCap, p, nbBatch);
  if (nbBatch > s.numBins) { // (the aligned rule is not monotonic in the ray count: the grid the buffers were sized for)
    // (p.looseT* stay the smaller count's: only a launch with relief reads them, and such a launch has the plain grid, which
    //  never has more bins for fewer rays and so never comes here)
    p.binT1 = s.binT1, p.binT2 = s.binT2, p.binTiles = s.binTiles;
    p.binScale1 = s.binScale1, p.binBias1 = s.binBias1, p.binScale2 = s.binScale2, p.binBias2 = s.binBias2;
    nbBatch = s.numBins;
  }
  p.numBins = nbBatch;
  // a surface source has no sort bins: its records lie in index order in the overflow region (gen_surface_kernel),
  // which the trace kernel reads as virtual bins of binCap rays
  const bool unbinned = L.gen == GEN_SURFACE || tiles;
  if (L.genWeights) // the batch's start weights, addressed by GLOBAL ray index like a host source's (gen_surface_kernel / a source model's generator writes them)
    p.hostWeights = c->dSurfRayWeights.p - first;
  if (unbinned)
    p.numBins = 0;
  if (L.relief)
    size_loose(c->geo.D, p); // (p.ovCap = the batch capacity: the tight bins' overflow region keeps its full size)
  else
    p.reliefCoarse = nullptr;
  {
    // bins per queue grab: ~1024 rays for big batches, but never so many that a small
    // batch (a short last one, a small launch) is handed to a few waves only
    const uint64_t waves = std::min<uint64_t>(L.grid, ((uint64_t)binRays + 255) / 256) * (VR_BLOCK / 64);
    // (a grab of the queue costs two dependent trips to memory: the packet kernels want long spans; the
    //  general kernel's rounds are long and its bounce chains uneven: shorter spans balance its tail)
    // (a round that straddles two spans mixes rays of two places: its packet query gives up — every failed query of a flat
    //  plane is one of these, 4.9 % of the rounds at 32 bins, 2 % at 64 — which costs the absorbing kernel nothing
    //  measurable but the general flat-scene kernels 3 % (their failed round also loses its follow-up segments))
    uint64_t spanBins = (uint64_t)mode_traits(L.traceMode).spanBins; // (16 general, 64 general flat-scene kernels, 32 the others)
    if (K.spanBins)
      spanBins = *K.spanBins;
    const uint64_t binsToDeal = unbinned ? ((uint64_t)binRays + p.binCap - 1) / p.binCap : nbBatch;
    p.chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(spanBins, binsToDeal / std::max<uint64_t>(waves * 2, 1)));
  }
  // One queue per XCD pays where neighbouring rounds share primitive records that do not fit an XCD's 4 MiB L2 and the
  // work per bin is even: flat scenes of more than ~10^5 primitives (measured, VR_QUEUES=1 / 8 on one box: C2 sticking
  // 0.1 15.62 -> 15.16 ms, C2 1.0 6.67 -> 6.62, plane 100^2 +-0; L2 hit rate of the C2 launch 74 -> 84 %, fabric reads
  // 9.0 -> 5.2 GB).  A structured scene is L2 resident anyway and its bins differ in cost — an eighth of the trench is
  // not an eighth of the work: trench3D +3 %, C5 +6 %: one queue.
  const bool flat = mode_traits(L.traceMode).xcdQueues; // (MODE_GENERAL_FLAT alone; the absorbing kernels have the single queue compiled in)
  p.numQueues = (flat && c->geo.numPrims > (1u << 17) && p.numBins >= 64u * VR_QUEUES * p.chunk) ? VR_QUEUES : 1u;
  if (K.numQueues)
    p.numQueues = *K.numQueues;
  return p;
}

// Can two launches share a generator pass?  (A stateful model's generator runs its own init: a pass of its own.  relief,
// binAlign: the generator's bins are laid out differently.)
static bool same_gen_group(const ParticleLaunch &a, const ParticleLaunch &b) {
  return !a.userGen && !b.userGen && a.absorb == b.absorb && a.params.ee == b.params.ee && a.params.eeGrid == b.params.eeGrid &&
         a.relief == b.relief && a.binAlign == b.binAlign;
}
// ... and is this launch alone in its group?  (The tile buckets serve one particle's kernel: run_batch.)
static bool tile_group_alone(const vr_context *c, const ParticleLaunch &L) {
  for (const ParticleLaunch &o : c->launches)
    if (&o != &L && same_gen_group(o, L))
      return false;
  return true;
}

// One batch of the ray stream: ONE generator pass straight into the sort bins, then the trace kernel of every
// particle of `group` over the same records (particles of a group share source distribution and record format).
static int run_batch(vr_context *c, const std::vector<const ParticleLaunch *> &group, uint64_t first, uint32_t count,
                     size_t &genNo, size_t &traceNo) {
  int rc = VR_OK;
  const ParticleLaunch &G = *group[0];
  const bool keepRng = !G.absorb; // records carry the RNG cursors
  // Tile buckets (vr_tile_buckets.hpp): a launch that is alone in its group.  It has no sort bins: the rays that are not
  // simple lie in the overflow region, the buckets behind it.  memsets, tile generator, tile kernel, then the
  // lattice-lanes kernel over the overflow region.
  const bool tiles = G.tileBuckets && group.size() == 1;
  const uint32_t binRays = tiles ? tile_bin_rays(count) : count;
  const TraceParams pg = batch_params(c, G, first, count, tiles);
  TileParams tp = G.tile;
  if (tiles) {
    tp.tileCount = c->dTileCount.p;
    tp.slotBase = pg.numBins * pg.binCap + pg.ovCap;
    tp.tileCap = c->knobs.tileCap.value_or(lattice_tile_capacity(count, G.tileSide, G.tileSrcArea));
    VR_HIP(c, hipMemsetAsync(tp.tileCount, 0, (size_t)tp.numTiles * 4, c->stream));
  }
  VR_HIP(c, hipMemsetAsync(pg.binCount, 0, (pg.reliefCoarse ? (size_t)pg.looseCntBase + pg.looseNumBins + 1 : (size_t)pg.numBins + 1) * 4, c->stream));
  hipEvent_t g0 = event_at(c->evG, 2 * genNo, c, rc), g1 = event_at(c->evG, 2 * genNo + 1, c, rc);
  if (rc != VR_OK)
    return rc;
  VR_HIP(c, hipEventRecord(g0, c->stream));
  if (G.userGen) { // a stateful model: its module's generator (init, then the source sample); a source model: its generator
    TraceParams pk = pg;
    SourceCtx sc = G.source;
    void *args[] = {&pk, &sc}; // (gen_state_kernel takes the first alone)
    const unsigned grid = std::min<unsigned>((count + VR_BLOCK - 1) / VR_BLOCK, (unsigned)c->numCUs * 8u);
    VR_HIP(c, hipModuleLaunchKernel(G.userGen, grid, 1, 1, VR_BLOCK, 1, 1, 0, c->stream, args, nullptr));
  } else if (tiles) {
    VR_HIP(c, launch_gen_tiles(pg, tp, (unsigned)c->numCUs * (unsigned)std::max(1, c->tileGenBlocks), c->stream));
  } else {
    VR_HIP(c, launch_gen(pg, G.gen, c->geo.D, keepRng, (unsigned)c->numCUs * 8u, c->stream));
  }
  VR_HIP(c, hipEventRecord(g1, c->stream));
  ++genNo;
  for (const ParticleLaunch *Lp : group) {
    const ParticleLaunch &L = *Lp;
    bool tight = true, loose = L.relief;
#ifdef VR_DIAG // (diagnostics: one of a relief scene's two launches alone — the result is incomplete)
    tight = !(L.relief && c->knobs.skipTight);
    loose = loose && !c->knobs.skipLoose;
#endif
    const TraceParams p = Lp == &G ? pg : batch_params(c, L, first, count);
    VR_HIP(c, hipMemsetAsync(p.workCounter, 0, VR_QUEUES * VR_QUEUE_STRIDE * 8, c->stream));
    if (p.spillCount)
      VR_HIP(c, hipMemsetAsync(p.spillCount, 0, 4, c->stream));
    hipEvent_t k0 = event_at(c->evK, 2 * traceNo, c, rc), k1 = event_at(c->evK, 2 * traceNo + 1, c, rc);
    if (rc != VR_OK)
      return rc;
    VR_HIP(c, hipEventRecord(k0, c->stream));
    // a small batch does not need the whole persistent grid: one wave per 64 rays is plenty
    const unsigned gridBatch = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(L.grid, ((uint64_t)binRays + 255) / 256));
    if (tiles) // (the buckets first: the rays it hands on join the overflow region the kernel below reads)
      VR_HIP(c, launch_tile_trace(p, tp, c->stream));
    if (tight && L.userKernel) {
      TraceParams pk = p;
      void *args[] = {&pk};
      VR_HIP(c, hipModuleLaunchKernel(L.userKernel, gridBatch, 1, 1, VR_BLOCK, 1, 1, trace_dynamic_lds(L.traceMode, p.smallBytes), c->stream,
                                      args, nullptr));
    } else if (tight) {
      VR_HIP(c, launch_trace(p, c->geo.D, c->geo.geo, L.kernelParticle, L.kernelMode, gridBatch, c->stream));
    }
    VR_HIP(c, hipEventRecord(k1, c->stream));
    ++traceNo;
    if (loose) {
      // the loose bins (the grazing rays, filed apart by the generator): the kernel for structured scenes over the second
      // set of bins — the same buffers from their loose parts on, a single queue
      TraceParams q = p;
      q.binCount = p.binCount + p.looseCntBase;
      q.slotRec = p.slotRec + (size_t)p.looseSlotBase * 8;
      q.numBins = p.looseNumBins;
      q.reliefCoarse = nullptr;
      q.numQueues = 1;
      {
        const uint64_t waves = std::min<uint64_t>(L.looseGrid, ((uint64_t)count / 8 + 255) / 256) * (VR_BLOCK / 64);
        q.chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(16, q.numBins / std::max<uint64_t>(waves * 2, 1)));
      }
      VR_HIP(c, hipMemsetAsync(q.workCounter, 0, VR_QUEUES * VR_QUEUE_STRIDE * 8, c->stream));
      hipEvent_t l0 = event_at(c->evK, 2 * traceNo, c, rc), l1 = event_at(c->evK, 2 * traceNo + 1, c, rc);
      if (rc != VR_OK)
        return rc;
      VR_HIP(c, hipEventRecord(l0, c->stream));
      const unsigned gridLoose = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(L.looseGrid, ((uint64_t)count / 4 + 255) / 256));
      VR_HIP(c, launch_trace(q, c->geo.D, c->geo.geo, L.kernelParticle, L.looseMode, gridLoose, c->stream));
      VR_HIP(c, hipEventRecord(l1, c->stream));
      ++traceNo;
    }
  }
  return VR_OK;
}

} // namespace vr

extern "C" {

int vr_apply_launch(vr_context *c) {
  if (!c)
    return VR_E_INVALID;
  if (!c->prepared)
    return fail(c, VR_E_STATE, "vr_apply_launch: call vr_apply_prepare first");
  VR_HIP(c, hipSetDevice(c->device));
  const uint32_t N = c->geo.numPrims;
  VR_HIP(c, hipMemsetAsync(c->dFluxAcc.p, 0, (size_t)c->accStride * c->accReplicas * c->totalPlanes() * 8, c->stream));
  VR_HIP(c, hipMemsetAsync(c->dCounters.p, 0, C_BLOCK * c->launches.size() * 8, c->stream));
  if (c->logActive) // (the sums, the dropped counter and the overflow flag)
    VR_HIP(c, hipMemsetAsync(c->dDataLog.p, 0, ((size_t)c->logTotal + 2) * 8, c->stream));
  VR_HIP(c, hipEventRecord(c->ev0, c->stream));
  // groups of particles that can share a generator pass: the same source distribution (cosine power: the rays of
  // index idx are then identical, gpu/raygTrace.hpp launches every particle with the apply's one seed) and the
  // same record format (with / without the RNG cursors)
  std::vector<std::vector<const ParticleLaunch *>> groups;
  for (const ParticleLaunch &L : c->launches) {
    bool placed = false;
    for (auto &g : groups)
      if (same_gen_group(*g[0], L)) {
        g.push_back(&L);
        placed = true;
        break;
      }
    if (!placed)
      groups.push_back({&L});
  }
  c->numGenLaunches = c->numTraceLaunches = 0;
  for (const auto &g : groups)
    for (uint64_t f = c->rayFirstLaunch; f < c->rayEndLaunch; f += c->batchCap) {
      const uint32_t cnt = (uint32_t)std::min<uint64_t>(c->batchCap, c->rayEndLaunch - f);
      int r = run_batch(c, g, f, cnt, c->numGenLaunches, c->numTraceLaunches);
      if (r != VR_OK)
        return r;
    }
  VR_HIP(c, hipEventRecord(c->ev1, c->stream));
  {
    const unsigned headroom = rank_headroom(c->worldSize);
    for (uint32_t l = 0; l < c->totalPlanes(); ++l)
      VR_HIP(c, launch_gather_flux(c->dFluxAcc.p + (size_t)l * c->accStride * c->accReplicas, c->accStride, c->accReplicas,
                                   c->dLeafOfOrig.p, N, c->fluxOut() + (size_t)l * N, headroom, c->dCounters.p + C_ACC_OVERFLOW, c->stream));
  }
  // flux statistics of the absorbing launches: unit weights, so both companion planes follow from the flux plane
  for (const ParticleLaunch &L : c->launches)
    if (L.stats && L.absorb) {
      unsigned long long *flux = c->fluxOut() + (size_t)L.dataBase * N;
      VR_HIP(c, launch_stats_fill_absorbing(flux, N, flux + (size_t)L.params.numData * N, flux + (size_t)(L.params.numData + 1u) * N, c->stream));
    }
  c->launched = true;
  return VR_OK;
}

static void info_from_counters(vr_trace_info &i, const unsigned long long *cnt) {
  i.totalRaysTraced = cnt[C_TRACES];
  i.nonGeometryHits = cnt[C_NONGEO];
  i.geometryHits = cnt[C_GEO];
  i.particleHits = cnt[C_PARTICLE];
  i.boundaryHits = cnt[C_BOUNDARY];
  i.reflections = cnt[C_REFLECTIONS];
  i.raysTerminated = cnt[C_TERMINATED];
  i.rngFullStates = cnt[C_TIER2];
}

int vr_apply_finish(vr_context *c) {
  if (!c)
    return VR_E_INVALID;
  if (!c->launched)
    return fail(c, VR_E_STATE, "vr_apply_finish: nothing launched");
  VR_HIP(c, hipSetDevice(c->device));
  VR_HIP(c, hipStreamSynchronize(c->stream));
  const size_t nPart = c->launches.size();
  std::vector<unsigned long long> all(C_BLOCK * nPart); // every particle's counter block (vr_types.hpp: C_*)
  VR_HIP(c, hipMemcpy(all.data(), c->dCounters.p, all.size() * 8, hipMemcpyDeviceToHost));
#ifdef VR_DIAG
  { // lane-occupancy diagnostics of a -DVR_DIAG build (see vr_trace_kernel.hpp)
    unsigned long long dg[32];
    VR_HIP(c, hipMemcpy(dg, c->dCounters.p + C_DIAG, sizeof(dg), hipMemcpyDeviceToHost));
    static const char *names[16] = {"rounds", "walk steps", "leaf prim tests", "packet visits", "packet prim tests",
                                    "state machine", "neighbour iters", "walk steps: unfinished", "refill reps", "wall init",
                                    "roulette", "credit", "pq attempts", "pq done", "visits: no child hit", "visits: both hit"};
    for (int k = 0; k < 16; ++k)
      if (dg[2 * k])
        std::fprintf(stderr, "diag %-18s wave-iters %12llu  lane-iters %14llu  (%.1f lanes)\n", names[k], dg[2 * k],
                     dg[2 * k + 1], (double)dg[2 * k + 1] / (double)dg[2 * k]);
    unsigned long long ph[16];
    VR_HIP(c, hipMemcpy(ph, c->dCounters.p + C_PHASE, sizeof(ph), hipMemcpyDeviceToHost));
    static const char *pn[16] = {"refill", "packets", "walk: search", "walk: leaf tests", "walls", "state machine + credit",
                                 "packet-query credit", "tail", "  (of state machine) neighbour loop", "  (of state machine) reflection + roulette; (absorbing kernels: of packets) packet query: record loads + box tests of the last level", "  (of state machine) from its start to the back-face test (vote, miss / wall branches, normal fetch)", "  (of state machine) boundary hit",
                                 "  (of state machine) up to the aggregation vote", "  (of state machine) up to the end counters", "  (of packets) packet query: descent of the 64-ary tree", "  (of packets) packet query: exact tests of the candidates"};
    double tot = 0;
    for (int k = 0; k < 8; ++k)
      tot += (double)ph[k];
    for (int k = 0; k < 16; ++k)
      if (ph[k])
        std::fprintf(stderr, "phase %-24s %5.1f %% of wave time\n", pn[k], 100.0 * (double)ph[k] / tot);
  }
#endif
  // A flux accumulator ran out of range (gather_flux_kernel): 2^23 = 8.39e6 weight units per primitive and data label
  // in one apply() — divided by the rank count rounded up to a power of two — is what int64 at 2^-40 holds (signed: the
  // multi-GPU all-reduce).  The reference's float sums stall near 2^24; these would wrap: the apply fails instead.
  if (all[C_ACC_OVERFLOW]) {
    c->launched = false;
    c->prepared = false;
    c->info.error = 1;
    ++c->runNumber; // (the apply happened, like one that ends in the reference's error flag: the seeds move on)
    return fail(c, VR_E_STATE, "flux accumulator overflow: a primitive collected more than 2^23 (8.39e6) weight units per rank-power-of-two "
                               "in one apply() (int64 fixed point, 2^-40 per unit) - result discarded; trace fewer rays per apply() "
                               "and sum the normalised results");
  }
  c->haveLog = false;
  if (c->logActive) {
    c->logHost.resize((size_t)c->logTotal + 2);
    VR_HIP(c, hipMemcpy(c->logHost.data(), c->dDataLog.p, c->logHost.size() * 8, hipMemcpyDeviceToHost));
    // a sum of the data log left 2^63 / ranks (rounded up to a power of two): raised by the add that saw it (gen_state_kernel)
    if (c->logHost[(size_t)c->logTotal + VR_LOG_OVERFLOW]) {
      c->launched = false;
      c->prepared = false;
      c->info.error = 1;
      ++c->runNumber;
      return fail(c, VR_E_STATE, "data log overflow: an entry collected more than 2^39 (5.5e11) units per rank-power-of-two in one "
                                 "apply() (int64 fixed point, 2^-24 per unit) - result discarded; log fewer rays per apply()");
    }
    c->logHost.resize((size_t)c->logTotal + 1); // (sums + [dropped])
    c->haveLog = true;
  }
  for (size_t q = 0; q < nPart; ++q) {
    // the walk's stack ran out (a tree deeper than SD + VR_STACK_GLOBAL levels of deferred children): the
    // result would be wrong, so the apply fails
    if (all[C_BLOCK * q + C_WALK_OVERFLOW]) {
      c->launched = false;
      c->prepared = false;
      return fail(c, VR_E_STATE, "BVH traversal stack overflow (degenerate tree), or a rank of a sharded apply failed: result discarded");
    }
  }
#ifdef VR_SELFCHECK
  {
    unsigned long long sc[C_CHECK_GEOM - C_CHECK + 1];
    VR_HIP(c, hipMemcpy(sc, c->dCounters.p + C_CHECK, sizeof(sc), hipMemcpyDeviceToHost));
    const unsigned long long *const ray = sc + (C_CHECK_RAY - C_CHECK);
    const unsigned long long pos = sc[C_CHECK_POS - C_CHECK], geom = sc[C_CHECK_GEOM - C_CHECK];
    std::fprintf(stderr, "[vr] self-check: %llu segments disagree with the escape-link walk\n", sc[0]);
    if (sc[0]) {
      float v[8];
      for (int k = 0; k < 8; ++k) {
        const uint32_t u = (uint32_t)ray[k];
        std::memcpy(&v[k], &u, 4);
      }
      std::fprintf(stderr, "[vr]   first: o %.9g %.9g %.9g d %.9g %.9g %.9g  t %.9g pos %u geom %d | ref t %.9g pos %u geom %d\n",
                   v[0], v[1], v[2], v[3], v[4], v[5], v[6], (unsigned)(pos >> 32), (int)(geom >> 32), v[7],
                   (unsigned)(pos & 0xFFFFFFFFu), (int)(geom & 0xFFFFFFFFu));
    }
  }
#endif
  float ms = 0.f;
  VR_HIP(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
  // per particle, and their sums in the context's TraceInfo
  unsigned long long sum[C_BLOCK] = {};
  for (size_t q = 0; q < nPart; ++q) {
    vr_trace_info &pi = c->launches[q].info;
    pi = vr_trace_info{};
    pi.numRays = c->numRaysLast;
    info_from_counters(pi, all.data() + C_BLOCK * q);
    for (size_t w = 0; w < C_BLOCK; ++w)
      sum[w] += all[C_BLOCK * q + w];
  }
  vr_trace_info &i = c->info;
  i.numRays = c->numRaysLast;
  info_from_counters(i, sum);
  i.timeTrace = ms * 1e-3;
  double kms = 0.0;
  for (size_t b = 0; b < c->numTraceLaunches; ++b) {
    float m = 0.f;
    VR_HIP(c, hipEventElapsedTime(&m, c->evK[2 * b], c->evK[2 * b + 1]));
    kms += m;
    if (c->knobs.printLaunches) // (diagnostics: a scene with relief runs two trace launches per batch)
      std::fprintf(stderr, "[vr] trace launch %zu: %.3f ms\n", b, m);
  }
  i.timeTraceKernel = kms * 1e-3;
  if (c->knobs.printLaunches) // (every launch's sort-bin grid of a full batch; cells in units of gridDelta)
    for (size_t q = 0; q < nPart; ++q) {
      const ParticleLaunch &L = c->launches[q];
      const BinGrid &g = L.binGrid;
      const double d = c->geo.gridDelta > 0.f ? (double)c->geo.gridDelta : 1.0;
      const ModeTraits kernel = mode_traits(L.kernelMode);
      std::fprintf(stderr, "[vr] sort bins: %u (%d x %d cells), VR_BIN_ALIGN %d, aligned %d, cell %.4g x %.4g gridDelta, mean rays per bin %.1f, particle %zu\n",
                   L.params.numBins, g.T1, g.T2, (int)c->knobs.binAlign, g.aligned, g.cell1 / d, g.cell2 / d, g.meanRays, q);
      // (the scene's fact, and whether this launch ran the uniform-disk kernel on it)
      std::fprintf(stderr, "[vr] uniform disks: scene %d, VR_UNIFORM_DISKS %d, launch %d, particle %zu\n", (int)c->uniformDisks,
                   (int)c->knobs.uniformDisks, (int)kernel.uniform, q);
      // (launch 1 above: a kernel of the uniform family ran; here: whether it was the planar one)
      std::fprintf(stderr, "[vr] planar disks: scene %d, VR_PLANAR_DISKS %d, launch %d, particle %zu\n", (int)c->planarDisks,
                   (int)c->knobs.planarDisks, (int)kernel.planar, q);
      // (... and whether it was that kernel's one-point-per-round form)
      std::fprintf(stderr, "[vr] planar disks: round: VR_PLANAR_ROUND %d, launch %d, particle %zu\n", (int)c->knobs.planarRound,
                   (int)kernel.planarRound, q);
      // (... and whether its candidates came from the lattice table)
      std::fprintf(stderr, "[vr] planar disks: lattice: scene %d, VR_PLANAR_LATTICE %d, launch %d, particle %zu\n", (int)c->planarLattice,
                   (int)c->knobs.planarLattice, (int)kernel.lattice, q);
      // (... and whether each lane tested its own four disks; scene: the host rule alone, lattice_lanes_rule)
      std::fprintf(stderr, "[vr] planar disks: lanes: scene %d, VR_LATTICE_LANE_TESTS %d, launch %d, particle %zu\n",
                   (int)L.latticeLanesScene, (int)c->knobs.latticeLaneTests, (int)kernel.latticeLanes, q);
      // (... in one word: the mode the launch reports and the kernel of the table it ran)
      std::fprintf(stderr, "[vr] kernel: traceMode %d, kernel mode %d, particle %zu\n", L.traceMode, L.kernelMode, q);
      // (the tile buckets: whether this launch ran them — it also has to be alone in its generator group — and the share
      //  of its rays that the lattice-lanes kernel traced instead: those the generator found not simple or found no room
      //  for, and those the tile kernel handed on)
      const bool ran = L.tileBuckets && tile_group_alone(c, L);
      const double rays = (double)std::max<uint64_t>(1, c->rayEndLaunch - c->rayFirstLaunch);
      std::fprintf(stderr, "[vr] tile buckets: VR_TILE_BUCKETS %d, launch %d, tiles %u (%d x %d of %d cells a side), slices %u, "
                           "other rays %.6f, handed on %.6f, particle %zu\n",
                   (int)c->knobs.tileBuckets, (int)ran, ran ? L.tile.numTiles : 0u, L.tile.tiles1, L.tile.tiles2, ran ? 1 << L.tile.shift : 0,
                   L.tile.slices, ran ? (double)all[C_BLOCK * q + C_TILE_FALLBACK] / rays : 0., ran ? (double)all[C_BLOCK * q + C_TILE_HANDED] / rays : 0., q);
    }

  const uint32_t *spillCount = launch_params(c, current_launch(c)).spillCount;
  if (c->knobs.printLaunches && spillCount) { // (diagnostics: rays the tight general relief kernel handed over)
    uint32_t sp = 0;
    if (hipMemcpy(&sp, spillCount, 4, hipMemcpyDeviceToHost) == hipSuccess)
      std::fprintf(stderr, "[vr] spilled rays (last batch): %u\n", sp);
  }
  double gms = 0.0;
  for (size_t b = 0; b < c->numGenLaunches; ++b) {
    float m = 0.f;
    VR_HIP(c, hipEventElapsedTime(&m, c->evG[2 * b], c->evG[2 * b + 1]));
    gms += m;
  }
  i.timeGenKernel = gms * 1e-3;
  i.timeBuild = c->buildSeconds;
  i.time = i.timeBuild + i.timeTrace;
  i.bvhRefits = (uint32_t)c->bvhRefits;
  i.bvhBuilds = c->bvhBuilds;
  for (auto &L : c->launches) {
    L.info.timeTrace = i.timeTrace;
    L.info.time = i.time;
    L.info.timeBuild = i.timeBuild;
  }
  ++c->runNumber; // rayTraceDisk.hpp:54
  c->haveSharedSeed = c->keepSharedSeed && c->haveSharedSeed;
  c->launched = false;
  c->prepared = false;
  c->haveResult = true;
  return VR_OK;
}

int vr_apply(vr_context *c) {
  int r = vr_apply_prepare(c);
  if (r != VR_OK)
    return r;
  r = vr_apply_launch(c);
  if (r != VR_OK)
    return r;
  return vr_apply_finish(c);
}

// Multi-GPU apply() behind the C ABI: this rank traces its contiguous share of the
// global ray indices, then the per-primitive int64 accumulators (exact, order-independent) and the
// seven counters are summed over all ranks by the caller's collective — RCCL over xGMI through
// vr_rccl_allreduce (libviennaray_amd_rccl.so), or anything else with the same signature.  Every
// rank ends with the full flux, bit-identical to the single-device run; runNumber advances on
// every rank (also one whose share is empty), so later applies keep using the same seeds.
int vr_apply_sharded(vr_context *c, int rank, int world, vr_allreduce_fn reduce, void *user) {
  if (!c || world < 1 || rank < 0 || rank >= world || (world > 1 && !reduce))
    return fail(c, VR_E_INVALID, "vr_apply_sharded: bad argument");
  VR_HIP(c, hipSetDevice(c->device));
  const uint64_t total = rays_of_apply(c);
  const uint64_t first = total * (uint64_t)rank / (uint64_t)world;
  const uint64_t last = total * (uint64_t)(rank + 1) / (uint64_t)world;
  const uint32_t N = c->geo.numPrims;
  // The all-reduce below sums whole counter blocks, so that the TraceInfo counters and both failure words travel together.
  static_assert(C_COUNT <= C_BLOCK && C_WALK_OVERFLOW < C_BLOCK && C_ACC_OVERFLOW < C_BLOCK,
                "the reduced counter blocks must carry the TraceInfo counters and both failure words");
  const size_t counterWords = C_BLOCK * c->numParticles();
  VR_HIP(c, c->dCounters.ensure(counterWords));
  c->haveSharedSeed = false;
  if (world > 1 && c->useRandomSeed) {
    // setUseRandomSeeds(true): every rank would draw its own seed and the shards would belong to different
    // streams.  Rank 0 draws, the others contribute 0, and the all-reduce hands the seed round.
    unsigned long long word = 0, *const seedWord = c->dCounters.p + C_SHARED_SEED;
    if (rank == 0) {
      std::random_device rd;
      word = (uint32_t)rd();
    }
    VR_HIP(c, hipMemcpyAsync(seedWord, &word, 8, hipMemcpyHostToDevice, c->stream));
    if (reduce(user, seedWord, 1, (void *)c->stream) != 0)
      return fail(c, VR_E_HIP, "vr_apply_sharded: the all-reduce callback failed (seed)");
    VR_HIP(c, hipMemcpyAsync(&word, seedWord, 8, hipMemcpyDeviceToHost, c->stream));
    VR_HIP(c, hipStreamSynchronize(c->stream));
    c->sharedSeed = (uint32_t)word;
    c->haveSharedSeed = true;
    c->keepSharedSeed = true; // (cleared below, after the launch)
  }
  int r = VR_OK;
  const uint32_t worldBefore = c->worldSize;
  c->worldSize = std::max<uint32_t>(c->worldSize, (uint32_t)world); // (head-room of the overflow check: the sums of all ranks fit int64)
  if (last > first) {
    c->rayFirst = first;
    c->rayCount = last - first;
    r = vr_apply_prepare(c);
    if (r == VR_OK)
      r = vr_apply_launch(c);
  } else {
    // an empty share: nothing to trace, but the scene is prepared like everywhere else (numRays, areas,
    // accumulator planes: the collective below must see the same buffer sizes on every rank)
    c->rayFirst = total; // (an empty range behind the last ray)
    c->rayCount = 1;
    r = vr_apply_prepare(c);
    if (r == VR_OK) {
      VR_HIP(c, hipMemsetAsync(c->fluxOut(), 0, (size_t)N * c->totalPlanes() * 8, c->stream));
      VR_HIP(c, hipMemsetAsync(c->dCounters.p, 0, counterWords * 8, c->stream));
      if (c->logActive)
        VR_HIP(c, hipMemsetAsync(c->dDataLog.p, 0, ((size_t)c->logTotal + 2) * 8, c->stream));
      VR_HIP(c, hipEventRecord(c->ev0, c->stream));
      VR_HIP(c, hipEventRecord(c->ev1, c->stream));
      c->numGenLaunches = c->numTraceLaunches = 0;
      c->launched = true;
    }
  }
  c->rayFirst = 0;
  c->rayCount = 0;
  c->haveSharedSeed = false;
  c->keepSharedSeed = false;
  c->worldSize = worldBefore;
  if (world > 1) {
    // A rank that failed above still enters the collectives when it can (zeros and a raised failure word) —
    // the others would hang in them otherwise.  The TraceInfo counters AND the failure words (C_WALK_OVERFLOW:
    // the walk's stack, or this; C_ACC_OVERFLOW) travel together, in counterWords: every rank fails together,
    // none returns VR_OK holding sums that include a discarded share.
    const std::string firstErr = c->err;
    const bool haveBuf = c->boundFlux ? c->boundFluxN == N * c->totalPlanes() : c->dFluxOrig.cap >= (size_t)N * c->totalPlanes();
    if (r != VR_OK) {
      if (!haveBuf)
        return r; // (failed before the accumulators existed: a configuration error, the same on every rank)
      const unsigned long long one = 1;
      (void)hipMemsetAsync(c->fluxOut(), 0, (size_t)N * c->totalPlanes() * 8, c->stream);
      (void)hipMemsetAsync(c->dCounters.p, 0, counterWords * 8, c->stream);
      (void)hipMemcpyAsync(c->dCounters.p + C_WALK_OVERFLOW, &one, 8, hipMemcpyHostToDevice, c->stream);
      if (c->logActive)
        (void)hipMemsetAsync(c->dDataLog.p, 0, ((size_t)c->logTotal + 2) * 8, c->stream);
    }
    // (the data log's sums travel with their dropped counter and overflow flag: the two words behind them; a shape that
    //  prepare refused is refused on every rank alike, so the ranks agree on logActive)
    if (reduce(user, c->fluxOut(), (size_t)N * c->totalPlanes(), (void *)c->stream) != 0 ||
        reduce(user, c->dCounters.p, counterWords, (void *)c->stream) != 0 ||
        (c->logActive && reduce(user, c->dDataLog.p, (size_t)c->logTotal + 2, (void *)c->stream) != 0))
      return fail(c, VR_E_HIP, "vr_apply_sharded: the all-reduce callback failed");
    if (r != VR_OK) {
      (void)hipStreamSynchronize(c->stream);
      c->err = firstErr;
      return r;
    }
  } else if (r != VR_OK) {
    return r;
  }
  return vr_apply_finish(c);
}

int vr_add_trace_info(vr_context *c, const vr_trace_info *o) {
  if (!c || !o)
    return VR_E_INVALID;
  vr_trace_info &i = c->info;
  i.totalRaysTraced += o->totalRaysTraced;
  i.nonGeometryHits += o->nonGeometryHits;
  i.geometryHits += o->geometryHits;
  i.particleHits += o->particleHits;
  i.boundaryHits += o->boundaryHits;
  i.reflections += o->reflections;
  i.raysTerminated += o->raysTerminated;
  i.rngFullStates += o->rngFullStates;
  return VR_OK;
}

} // extern "C"
