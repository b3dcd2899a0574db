// vr_prepare.cpp — vr_apply_prepare: everything an apply() needs before its kernels run, one stage after the other
// (prepare_one), for every particle of the apply: each stage reads the ParticleSpec it is given.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "vr_context.hpp"
#include "vr_lattice_tiles.hpp"
#include "vr_particles.hpp"
#include "vr_planar_disks.hpp"
#include "vr_planar_lattice.hpp"
#include "vr_uniform_disks.hpp"

namespace vr {

// ---- run ----------------------------------------------------------------------
static int effective_direction(const vr_context *c) {
  if (c->sourceDirection >= 0)
    return c->sourceDirection;
  return c->geo.D == 2 ? VR_POS_Y : VR_POS_Z; // rayTrace.hpp:166-167
}

// ---- apply() set-up: prepare_one and its stages ------------------------------------------------------------------

// what the stages of one prepare_one hand on to each other
struct PrepareState {
  bool stateful = false;    // a stateful run-time model (its generator, per-ray state and material ids)
  bool flatScene = false;   // the surface shown to the source lies in one plane and the scene box is thin along its axis
  bool smallScene = false;  // the whole scene goes into LDS (MODE 4)
  bool heightField = false; // the height field over the source plane is built (the frame's VR_F_HF_*)
  const int32_t *dMaterial = nullptr; // a stateful model's material ids (the frame's VR_F_MAT_*)
  bool logs = false;        // the model has a log_data hook and the apply a data-log shape (the frame's VR_F_LOG_*)
};

// the largest coordinate of the BVH's root box (at least 1e-3): the scale of the float rounding the pads cover
static float scene_scale(const vr_context *c) {
  float scale = 1e-3f;
  for (int k = 0; k < 3; ++k)
    scale = std::max(scale, std::max(std::fabs(c->sceneLo[k]), std::fabs(c->sceneHi[k])));
  return scale;
}

// Sort-bin grid for a batch of `count` rays whose overflow region has `ovCap` slots: far-plane cells holding ~raysPerBin
// rays each.  A 3-D launch on disks (`align`: VR_BIN_ALIGN and the launch's geometry) gets the grid aligned with the disk
// lattice where vr_bin_grid.hpp's rule can be met, every other one the plain grid.  The lattice's phase is the smallest
// disk centre per axis: on a cloud made from a level set that IS a lattice line, on any other cloud any phase will do.
BinGrid size_bins(const vr_context *c, bool align, uint64_t count, uint32_t ovCap, TraceParams &p, uint32_t &numBins) {
  const int D = c->geo.D;
  const BinGrid plain = bin_grid_plain(D, count, c->raysPerBin);
  BinGrid g = plain;
  if (align && D == 3 && c->geo.geo == 0 && c->geo.gridDelta > 0.f) {
    BinGridIn in;
    in.rays = count;
    in.perBin = c->raysPerBin;
    in.binCap = p.binCap;
    in.ovCap = ovCap;
    in.lo1 = c->bbLo[c->ts[1]];
    in.hi1 = c->bbHi[c->ts[1]];
    in.lo2 = c->bbLo[c->ts[2]];
    in.hi2 = c->bbHi[c->ts[2]];
    in.phase1 = c->geo.minC[c->ts[1]];
    in.phase2 = c->geo.minC[c->ts[2]];
    in.pitch = c->geo.gridDelta;
    bin_grid_aligned(in, g); // (false: g is still the plain grid)
  }
  if (!g.aligned) { // (diagnostics: the plain grid's cells)
    g.cell1 = ((double)c->bbHi[c->ts[1]] - (double)c->bbLo[c->ts[1]]) / g.T1;
    g.cell2 = D == 3 ? ((double)c->bbHi[c->ts[2]] - (double)c->bbLo[c->ts[2]]) / g.T2 : 0.;
  }
  p.binT1 = g.T1;
  p.binT2 = g.T2;
  p.binTiles = g.tiles;
  p.binScale1 = g.scale1;
  p.binBias1 = g.bias1;
  p.binScale2 = g.scale2;
  p.binBias2 = g.bias2;
  // (the loose bins of a relief scene keep the plain grid's cells: size_loose)
  p.looseT1 = std::max(1, plain.T1 / 3);
  p.looseT2 = D == 2 ? 1 : std::max(1, plain.T2 / 3);
  numBins = g.numBins;
  return g;
}

// The LOOSE bins of a scene with relief (TraceParams, round 4): a grid a third as fine per axis as the PLAIN tight one
// (size_bins left its cells per axis in p.looseT*) — they hold the grazing rays, about a tenth of all — whose cursors and
// record slots (+ an overflow region of p.ovCap slots) lie behind the tight bins' in the same two buffers.
void size_loose(int D, TraceParams &p) {
  if (D == 2) {
    p.looseT2 = 1;
    p.looseTiles = 1;
    p.looseNumBins = (uint32_t)p.looseT1;
  } else {
    p.looseTiles = (p.looseT1 + 7) / 8;
    p.looseNumBins = (uint32_t)p.looseTiles * (uint32_t)((p.looseT2 + 7) / 8) * 64u;
  }
  p.looseCntBase = (p.numBins + 1u + 3u) & ~3u;
  p.looseSlotBase = p.numBins * p.binCap + p.ovCap;
}

// The ray-stream buffers for batches of `cap` rays: the sort-bin grid (into p.binT*), the record slots (bins + overflow
// region) and the bin-cursor words; with relief, the loose bins and their overflow region behind the tight ones.
struct StreamExtent {
  uint32_t numBins = 0;
  size_t slots = 0, cntWords = 0;
  size_t looseSlots = 0; // (relief) record slots of the loose bins + their overflow region
  BinGrid grid;
};
static StreamExtent stream_extent(const vr_context *c, bool align, uint32_t cap, bool relief, TraceParams &p) {
  const int D = c->geo.D;
  StreamExtent e;
  e.grid = size_bins(c, align, cap, cap, p, e.numBins);
  e.slots = (size_t)e.numBins * p.binCap + cap;
  e.cntWords = (size_t)e.numBins + 1;
  if (relief) {
    TraceParams q = p;
    q.numBins = e.numBins;
    q.ovCap = cap;
    size_loose(D, q);
    e.looseSlots = (size_t)q.looseNumBins * p.binCap + cap;
    e.slots = (size_t)q.looseSlotBase + e.looseSlots;
    e.cntWords = (size_t)q.looseCntBase + q.looseNumBins + 1;
  }
  return e;
}

// checkSettings (rayTraceDisk.hpp:196-217): the reference logs and carries on; with nothing to trace we stop and report
// through the error flag.
static int check_settings(vr_context *c) {
  c->info = vr_trace_info{};
  if (c->specs.empty()) {
    c->info.error = 1;
    return fail(c, VR_E_INVALID, "No particle was specified in rayTrace. Aborting.");
  }
  if (c->geo.numPrims == 0) {
    c->info.error = 1;
    return fail(c, VR_E_INVALID, "No geometry was passed to rayTrace. Aborting.");
  }
  const int dir = effective_direction(c);
  if (c->geo.D == 2 && (dir == VR_POS_Z || dir == VR_NEG_Z)) {
    c->info.error = 1;
    return fail(c, VR_E_INVALID, "Invalid source direction in 2D geometry. Aborting.");
  }
  if (c->geo.geo == 0 && c->geo.diskRadius > c->geo.gridDelta)
    c->info.warning = 1;
  // (a surface source divides the ray index by the rays per point in 32 bits: the index is tea3's 32-bit input anyway)
  if (c->src.kind == SourceKind::Surface && rays_of_apply(c) > 0xFFFFFFFFull) {
    c->info.error = 1;
    return fail(c, VR_E_INVALID, "surface source: points x rays per point exceeds the 32-bit ray index of one apply");
  }
  return VR_OK;
}

// host_sort_plane for a device-resident geometry: the histogram is made where the primitives are (launch_sort_plane),
// 512 doubles come back and the fullest slice is picked as the host function picks it.  (The sums are taken in another
// order than the host threads take them: the plane may differ in its last bits; it only orders work.)
static int device_sort_plane(vr_context *c, int axis, float fallback, float *coord, float *modeShare) {
  const HostGeometry &g = c->geo;
  const float lo = g.minC[axis], hi = g.maxC[axis];
  *modeShare = 1.f;
  if (g.numPrims == 0 || !(hi > lo)) {
    *coord = g.numPrims ? lo : fallback;
    return VR_OK;
  }
  constexpr int SL = 256;
  const size_t scratch = sort_plane_partials_entries();
  VR_HIP(c, c->dSortPlane.ensure(scratch + 2 * SL));
  double h[2 * SL];
  VR_HIP(c, launch_sort_plane(g.geo, c->dDisk4.p, c->dNormal3.p, c->dVerts.p, c->dTris.p, g.numPrims, axis, lo, hi,
                              c->dSortPlane.p, c->dSortPlane.p + scratch, c->stream));
  VR_HIP(c, hipMemcpyAsync(h, c->dSortPlane.p + scratch, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  VR_HIP(c, hipStreamSynchronize(c->stream));
  const double *w = h, *wh = h + SL;
  int best = 0;
  double total = w[0];
  for (int k = 1; k < SL; ++k) {
    total += w[k];
    if (w[k] > w[best])
      best = k;
  }
  if (total > 0.)
    *modeShare = (float)(w[best] / total);
  *coord = w[best] > 0. ? (float)(wh[best] / w[best]) : fallback;
  return VR_OK;
}

// bounding box, trace settings, walls, boundary conditions (rayTraceDisk.hpp:21-27), source area and the sort plane
static int setup_source_frame(vr_context *c) {
  const int D = c->geo.D;
  for (int k = 0; k < 3; ++k) {
    c->bbLo[k] = c->geo.minC[k];
    c->bbHi[k] = c->geo.maxC[k];
  }
  host_adjust_bbox(c->bbLo, c->bbHi, D, effective_direction(c), c->geo.geo == 0 ? c->geo.diskRadius : c->geo.gridDelta);
  c->ts = host_trace_settings(effective_direction(c));
  {
    Tri walls[8];
    host_build_walls(c->bbLo, c->bbHi, c->ts[1], c->ts[2], walls);
    float *tbl = c->wallsHost; // (uploaded with the launch's scalar frame: write_launch_frame)
    for (int i = 0; i < 8; ++i) {
      std::memcpy(tbl + 12 * i, walls[i].v0, 12);
      std::memcpy(tbl + 12 * i + 3, walls[i].e1, 12);
      std::memcpy(tbl + 12 * i + 6, walls[i].e2, 12);
      std::memcpy(tbl + 12 * i + 9, walls[i].Ng, 12);
    }
  }
  // rayBoundary.hpp:23-25: conditions are picked by AXIS
  c->boundaryConds[0] = c->bcs[c->ts[1]];
  c->boundaryConds[1] = (D == 2 && c->ts[2] >= 2) ? 0 : c->bcs[c->ts[2]];
  // SourceRandom::getSourceArea (raySourceRandom.hpp:40-47)
  const int f = c->ts[1], s = c->ts[2];
  c->sourceArea = D == 2 ? (c->bbHi[f] - c->bbLo[f]) : (c->bbHi[f] - c->bbLo[f]) * (c->bbHi[s] - c->bbLo[s]);
  const float fallback = c->ts[3] ? c->geo.minC[c->ts[0]] : c->geo.maxC[c->ts[0]];
  // (a device-resident mesh under VR_HOST_BUILD, the validation path: the host function on the downloaded mirror)
  const bool hostMesh = c->geo.geo == 1 && c->knobs.hostBuild;
  if (c->geoOnDevice && !hostMesh)
    return device_sort_plane(c, c->ts[0], fallback, &c->keyCoord, &c->keyShare);
  VR_TRY(ensure_host_geometry(c));
  c->keyCoord = host_sort_plane(c->geo, c->ts[0], fallback, &c->keyShare);
  return VR_OK;
}

// exposed area of every primitive, resident on the device for normalizeFlux
// (computeDiskAreas, rayGeometryDisk.hpp:266-354: one thread per disk; triangle areas come
// with the mesh, rayGeometryTriangle.hpp:145-176)
static int compute_areas(vr_context *c) {
  const uint32_t N = c->geo.numPrims;
  VR_HIP(c, c->dAreas.ensure(N));
  c->diskAreasHostValid = false;
  if (c->geo.geo == 0) {
    AreaParams ap{};
    ap.D = c->geo.D;
    ap.firstDir = c->ts[1];
    ap.secondDir = c->ts[2];
    // rayGeometryDisk.hpp:281-284 indexes the 2-entry BC array by AXIS; axis 2 is out of
    // range there, entry 1 is used for it
    ap.bcFirst = c->boundaryConds[c->ts[1] > 1 ? 1 : c->ts[1]];
    ap.bcSecond = c->boundaryConds[c->ts[2] > 1 ? 1 : c->ts[2]];
    for (int k = 0; k < 3; ++k) {
      ap.minC[k] = c->geo.minC[k];
      ap.maxC[k] = c->geo.maxC[k];
    }
    if (c->knobs.hostBuild) {
      const int r = ensure_host_geometry(c);
      if (r != VR_OK)
        return r;
      host_disk_areas(c->geo, ap, c->diskAreas);
      VR_HIP(c, hipMemcpy(c->dAreas.p, c->diskAreas.data(), (size_t)N * 4, hipMemcpyHostToDevice));
      c->diskAreasHostValid = true;
    } else {
      VR_HIP(c, launch_disk_areas(c->dDisk4.p, c->dNormal3.p, N, ap, c->dAreas.p, c->stream));
    }
  } else if (c->geoOnDevice) {
    // (launch_pack_mesh left them in dTriAreas, which nothing else writes: no upload)
    VR_HIP(c, hipMemcpyAsync(c->dAreas.p, c->dTriAreas.p, (size_t)N * 4, hipMemcpyDeviceToDevice, c->stream));
  } else {
    VR_HIP(c, hipMemcpyAsync(c->dAreas.p, c->geo.triAreas.data(), (size_t)N * 4, hipMemcpyHostToDevice, c->stream));
    VR_HIP(c, hipStreamSynchronize(c->stream));
  }
  c->areasValid = true;
  return VR_OK;
}

// per-primitive sticking from the material map (gpu::Particle-style, rayParticle.hpp:208-218), the particle's own buffer:
// one kernel over the resident leaf order and material ids (host-set ids are uploaded first: ensure_device_material_ids),
// so neither the order nor the ids come back to the host
static int prepare_sticking(vr_context *c, const ParticleSpec &sp, ParticleLaunch &L) {
  L.params.primSticking = nullptr;
  if (sp.matIds.empty())
    return VR_OK;
  VR_TRY(ensure_device_material_ids(c));
  const uint32_t N = c->geo.numPrims;
  const size_t M = sp.matIds.size();
  L.matTableHost.resize(2 * M);
  std::memcpy(L.matTableHost.data(), sp.matIds.data(), M * 4);
  std::memcpy(L.matTableHost.data() + M, sp.matVals.data(), M * 4);
  VR_HIP(c, L.matTable.ensure(2 * M));
  VR_HIP(c, hipMemcpyAsync(L.matTable.p, L.matTableHost.data(), 2 * M * 4, hipMemcpyHostToDevice, c->stream));
  VR_HIP(c, L.primSticking.ensure(N));
  VR_HIP(c, launch_prim_sticking(c->dOrder.p, c->dMaterialIds.p, c->materialCount, L.matTable.p,
                                 reinterpret_cast<const float *>(L.matTable.p + M), (unsigned)M, sp.sticking, N,
                                 L.primSticking.p, c->stream));
  L.params.primSticking = L.primSticking.p;
  return VR_OK;
}

// Trace::setGlobalData.  Host-set vectors only: every vector padded to one stride, one upload.  With vectors that were
// set from the device (their rows are in place since they were set), only the host-set rows that changed go up, each into
// its own row.
static int upload_global_data(vr_context *c) {
  c->globalRows.resize(c->globalVecs.size());
  if (!c->anyGlobalOnDevice()) {
    if (c->globalRowsLaid) // (row kernels of earlier device sets may still be on their way)
      VR_HIP(c, hipStreamSynchronize(c->stream));
    uint32_t stride = 0;
    for (const auto &v : c->globalVecs)
      stride = std::max<uint32_t>(stride, (uint32_t)v.size());
    c->globalStride = stride;
    c->globalRowsLaid = 0;
    if (stride && !c->globalVecs.empty()) {
      std::vector<float> flat((size_t)stride * c->globalVecs.size(), 0.f);
      for (size_t v = 0; v < c->globalVecs.size(); ++v)
        std::copy(c->globalVecs[v].begin(), c->globalVecs[v].end(), flat.begin() + v * stride);
      VR_HIP(c, c->dGlobalVec.ensure(flat.size()));
      VR_HIP(c, hipMemcpy(c->dGlobalVec.p, flat.data(), flat.size() * 4, hipMemcpyHostToDevice));
      c->globalRowsLaid = (uint32_t)c->globalVecs.size();
    }
    for (size_t v = 0; v < c->globalRows.size(); ++v) {
      c->globalRows[v].len = (uint32_t)c->globalVecs[v].size();
      c->globalRows[v].pending = false;
    }
  } else {
    uint32_t stride = 0;
    for (const auto &r : c->globalRows)
      stride = std::max(stride, r.len);
    VR_TRY(lay_global_rows(c, (uint32_t)c->globalRows.size(), stride));
    bool pending = false;
    for (const auto &r : c->globalRows)
      pending = pending || (!r.onDevice && r.pending);
    if (pending) // (lay_global_rows' fill of a new row comes first)
      VR_HIP(c, hipStreamSynchronize(c->stream));
    std::vector<float> row(pending ? c->globalStride : 0);
    for (size_t v = 0; v < c->globalRows.size(); ++v) {
      if (c->globalRows[v].onDevice || !c->globalRows[v].pending)
        continue;
      std::fill(std::copy(c->globalVecs[v].begin(), c->globalVecs[v].end(), row.begin()), row.end(), 0.f);
      VR_HIP(c, hipMemcpy(c->dGlobalVec.p + v * (size_t)c->globalStride, row.data(), row.size() * 4, hipMemcpyHostToDevice));
      c->globalRows[v].pending = false;
    }
  }
  if (!c->globalScalars.empty()) {
    VR_HIP(c, c->dGlobalScalars.ensure(c->globalScalars.size()));
    VR_HIP(c, hipMemcpy(c->dGlobalScalars.p, c->globalScalars.data(), c->globalScalars.size() * 4, hipMemcpyHostToDevice));
  }
  c->globalDirty = false;
  return VR_OK;
}

// the particle's kernel variant (absorbing, built-in, extended, stateful), the small-scene layout and whether the scene
// is flat
static int choose_particle_kernel(vr_context *c, const ParticleSpec &sp, ParticleLaunch &L, PrepareState &S) {
  TraceParams &p = L.params;
  const uint32_t N = c->geo.numPrims;
  // flux statistics: the two companion planes count against the planes one particle may have
  L.stats = c->fluxStats;
  if (L.stats && sp.numData > (uint32_t)(VR_MAX_LABELS - VR_STAT_PLANES))
    return fail(c, VR_E_INVALID, ("flux statistics (vr_set_flux_statistics) take " + std::to_string(VR_STAT_PLANES) + " of a particle's " +
                                  std::to_string(VR_MAX_LABELS) + " accumulator planes (VR_MAX_LABELS): a particle model may have at most " +
                                  std::to_string(VR_MAX_LABELS - VR_STAT_PLANES) + " data labels with statistics on, this one has " +
                                  std::to_string(sp.numData)).c_str());
  // ABSORB: every hit takes the whole weight -> nothing after the first
  // surface hit is observable
  L.absorb = sp.sticking >= 1.f;
  for (float v : sp.matVals)
    L.absorb = L.absorb && v >= 1.f;
  // the extended kernel (vr_particles.hpp) serves everything beyond the two built-in particles
  const bool extended = sp.kernelKind >= VR_PARTICLE_CONED_COSINE || c->useWdist || sp.meanFreePath > 0.f;
  if (extended)
    L.absorb = false;
  if (c->src.rays_start_weighted())
    L.absorb = false; // (the absorbing kernels credit unit weights)
  // (the rare, register-hungry options — coned-cosine model, WDIST crediting, mean free path — have an instantiation
  //  of their own: multi-label and per-material particles should not pay for them)
  bool extFull = Particles::needsFull(sp.kernelKind) || c->useWdist || sp.meanFreePath > 0.f;
  const UserModel *um = sp.userModel >= 0 ? &c->userModels[sp.userModel] : nullptr;
  if (um) {
    if (extFull && !um->needsFull)
      return fail(c, VR_E_INVALID, "this particle model was registered without VR_MODEL_NEEDS_FULL: its code object has no "
                                   "kernel with WDIST crediting / mean-free-path scattering");
    extFull = um->needsFull;
    if (um->numState > 0 && !c->src.admits_stateful_model())
      return fail(c, VR_E_INVALID, "a stateful particle model (numState > 0) runs its init on the device before the source "
                                   "sample: SourceRandom only (plain or with a primary direction), not SourceGrid, a host "
                                   "source, a surface source or a source model");
  }
  S.stateful = um && um->numState > 0;
  S.logs = S.stateful && c->logActive && um->logRows > 0;
  L.kernelParticle = extended ? (extFull ? (int)P_EXT_FULL : (int)P_EXT) : sp.kernelKind;
  // a scene of a few hundred primitives goes into LDS as a whole (MODE 4: the general kernel — also for
  // absorbing particles — of whatever particle): pair nodes, records, neighbourhood, accumulators (one plane
  // per data label), per-material sticking
  {
    const uint32_t recB = c->geo.geo == 0 ? 32u : 64u;
    uint32_t off[6], o = 0, nbTotal = 0;
    if (c->geo.geo == 0)
      nbTotal = c->nbTotal;
    auto put = [&](int k, size_t bytes) {
      off[k] = o;
      o += (uint32_t)((bytes + 15) & ~(size_t)15);
    };
    put(0, (size_t)c->numNodes * 32);
    put(1, (size_t)N * recB);
    put(2, ((size_t)N + 1) * 4);
    put(3, (size_t)nbTotal * 4);
    put(4, (size_t)N * 8 * (sp.numData + (c->fluxStats ? (uint32_t)VR_STAT_PLANES : 0u)));
    put(5, p.primSticking ? (size_t)N * 4 : 0);
    S.smallScene = o <= VR_SMALL_LDS && c->numNodes > 0 && c->knobs.smallScene;
    for (int k = 0; k < 6; ++k)
      p.smallOff[k] = off[k];
    p.smallNb = nbTotal;
    p.smallBytes = (o + 255u) & ~255u;
    if (S.smallScene)
      L.absorb = false; // (ray records with the RNG cursors: the general kernel reads them)
  }
  // Flux statistics: an absorbing launch keeps its kernel (unit weights: its companion planes are filled from the flux
  // plane after the gather, vr_apply_launch); every other launch runs the extended instantiation with the statistics
  // compiled in — the built-in particles as models 0 / 1 of the registry
  if (L.stats && !L.absorb)
    L.kernelParticle = extFull ? (int)P_EXT_FULL_STATS : (int)P_EXT_STATS;
  S.flatScene = c->keyShare >= 0.95f && (c->sceneHi[c->ts[0]] - c->sceneLo[c->ts[0]]) <= 0.25f * c->geo.gridDelta;
  return VR_OK;
}

// ---- flat WITH RELIEF?  (DESIGN.md 5.2 "relief packets")  The flat-scene kernels owe their speed to the packet
// query, and the query clips its rays to the SCENE box: half a grid cell of relief lets the grazing rays of a wave
// stretch its box over hundreds of cells.  Where the scene is thin along the source axis and the relief field says that
// few rays would be grazing ones (ReliefParams::stats), the rays are sorted by their predicted first hit, the grazing ones are filed apart
// (bin_of_relief, vr_generate.hpp) and the query clips to the LOCAL relief (relief_clip, vr_packet_query.hpp): MODE 5 / 6.
static int build_relief_field(vr_context *c, const ParticleSpec &sp, ParticleLaunch &L, const PrepareState &S) {
  const Knobs &K = c->knobs;
  TraceParams &p = L.params;
  const int D = c->geo.D;
  const float travel = K.reliefTravel;
  L.relief = false;
  const float thickScene = c->sceneHi[c->ts[0]] - c->sceneLo[c->ts[0]];
  const bool plainSource = c->src.is_plain(c->usePrimaryDirection);
  const int tightMode = L.absorb ? MODE_ABSORB_RELIEF : MODE_GENERAL_RELIEF; // (the catalogue has MODE_RESUME where it has the latter)
  const bool kernelOk = trace_kernel_exists(KERNELS_LIBRARY, D, c->geo.geo, trace_kernel_particle(L.kernelParticle, tightMode), tightMode);
  const bool want = !S.flatScene && !S.smallScene && plainSource && kernelOk && sp.userModel < 0 && c->geo.gridDelta > 0.f &&
                    thickScene <= K.reliefMaxThick * c->geo.gridDelta && !K.noRelief;
  if (want) {
    const bool stale = c->rfBuild != c->bvhBuilds || c->rfAxes[0] != c->ts[0] || c->rfAxes[1] != c->ts[1] ||
                       c->rfAxes[2] != c->ts[2] || c->rfAxes[3] != c->ts[3] || c->rf.travel != travel * c->geo.gridDelta;
    if (stale) {
      ReliefParams &q = c->rf;
      q.prims = c->dPrims.p;
      q.n = c->geo.numPrims;
      q.geo = c->geo.geo;
      q.ax = c->ts[0];
      q.a1 = c->ts[1];
      q.a2 = c->ts[2];
      const float ext1 = c->sceneHi[q.a1] - c->sceneLo[q.a1], ext2 = D == 3 ? c->sceneHi[q.a2] - c->sceneLo[q.a2] : 0.f;
      const float tile = std::max(K.reliefTile * c->geo.gridDelta, std::max(ext1, ext2) / 1024.f); // (fine tile)
      q.tile = tile;
      q.invTile = 1.f / tile;
      q.lo1 = c->sceneLo[q.a1];
      q.lo2 = D == 3 ? c->sceneLo[q.a2] : 0.f;
      q.nx = std::max(1, std::min(1024, (int)std::ceil(ext1 / tile)));
      q.ny = D == 3 ? std::max(1, std::min(1024, (int)std::ceil(ext2 / tile))) : 1;
      q.k = K.reliefCoarseK.value_or(std::max(2, (std::max(q.nx, q.ny) + 255) / 256));
      q.cnx = (q.nx + q.k - 1) / q.k;
      q.cny = (q.ny + q.k - 1) / q.k;
      q.pad = 1e-5f * scene_scale(c);
      q.travel = travel * c->geo.gridDelta;
      q.emptyMid = c->keyCoord;
      VR_HIP(c, c->dRfRawLo.ensure((size_t)q.nx * q.ny));
      VR_HIP(c, c->dRfRawHi.ensure((size_t)q.nx * q.ny));
      VR_HIP(c, c->dRfFine.ensure((size_t)q.nx * q.ny * 2));
      VR_HIP(c, c->dRfCoarse.ensure((size_t)q.cnx * q.cny * 2));
      VR_HIP(c, c->dRfStats.ensure(2));
      q.rawLo = c->dRfRawLo.p;
      q.rawHi = c->dRfRawHi.p;
      q.fine = c->dRfFine.p;
      q.coarse = c->dRfCoarse.p;
      q.stats = c->dRfStats.p;
      VR_HIP(c, launch_relief_field(q, c->stream));
      uint32_t st[2] = {0, 0};
      VR_HIP(c, hipMemcpyAsync(st, q.stats, sizeof(st), hipMemcpyDeviceToHost, c->stream));
      VR_HIP(c, hipStreamSynchronize(c->stream));
      c->rfLooseShare = st[0] ? (float)st[1] / 4096.f / (float)st[0] : 1.f;
      c->rfBuild = c->bvhBuilds;
      for (int k = 0; k < 4; ++k)
        c->rfAxes[k] = c->ts[k];
    }
    // (the share of a cosine source's rays that the generator would file as loose, from the coarse tiles' thickness:
    //  where most rays are loose the structured-scene kernels do the work anyway, without the second launch)
    L.relief = c->rfLooseShare <= K.reliefShare;
  }
  p.reliefCoarse = L.relief ? c->rf.coarse : nullptr;
  p.rcLo1 = c->rf.lo1;
  p.rcLo2 = c->rf.lo2;
  p.rcInvT = L.relief ? c->rf.invTile / (float)c->rf.k : 0.f;
  p.rcNx = c->rf.cnx;
  p.rcNy = c->rf.cny;
  p.reliefTravel = travel * c->geo.gridDelta;
  // the tile walk of relief_clip starts where the ray enters the SCENE box: a ray that would cross more than `steps`
  // tiles on its way through it is filed as loose too
  p.reliefTanMax = thickScene > 0.f ? K.reliefSteps * c->rf.tile / thickScene : 3.0e38f;
  // (2 look-ups: tight launch -0.1 ms, generator +0.4 ms per 1e8 rays — a random 8-byte gather per ray is a 128-byte line from L2)
  p.reliefLookups = K.reliefLookups;
  return VR_OK;
}

// accumulators: one plane per data label of all particles, each replicated accReplicas times
static int ensure_accumulators(vr_context *c) {
  const uint32_t N = c->geo.numPrims;
  if (c->accPlanes != c->totalPlanes()) {
    VR_HIP(c, c->dFluxAcc.ensure((size_t)c->accStride * c->accReplicas * c->totalPlanes()));
    VR_HIP(c, c->dFluxOrig.ensure((size_t)N * c->totalPlanes()));
    c->accPlanes = c->totalPlanes();
  }
  if (c->boundFlux && c->boundFluxN != N * c->totalPlanes())
    return fail(c, VR_E_STATE, "bound accumulator buffer does not hold numPrims x numData int64 (flux statistics: two more planes per particle)");
  return VR_OK;
}

// the sources whose payload comes up from the host: SourceGrid origins, host rays (+ draw counts, weights)
static int upload_source_data(vr_context *c) {
  RaySource &src = c->src;
  if (src.kind == SourceKind::Grid)
    VR_HIP(c, c->dGrid.upload(src.gridPoints.data(), src.gridPoints.size()));
  if (src.kind == SourceKind::HostRays) {
    VR_HIP(c, c->dHostOrg.ensure(src.hostOrg.size()));
    VR_HIP(c, c->dHostDir.ensure(src.hostDir.size()));
    VR_HIP(c, hipMemcpy(c->dHostOrg.p, src.hostOrg.data(), src.hostOrg.size() * 4, hipMemcpyHostToDevice));
    VR_HIP(c, hipMemcpy(c->dHostDir.p, src.hostDir.data(), src.hostDir.size() * 4, hipMemcpyHostToDevice));
    if (!src.hostDraws.empty())
      VR_HIP(c, c->dHostDraws.upload(src.hostDraws.data(), src.hostDraws.size()));
    if (!src.hostWeights.empty())
      VR_HIP(c, c->dHostWeights.upload(src.hostWeights.data(), src.hostWeights.size()));
  }
  src.sourceDirty = false;
  return VR_OK;
}

// ---- ray stream: the apply's ray range, in batches of up to 2^27 rays; larger launches run several batches ----------
static int size_ray_stream(vr_context *c, ParticleLaunch &L, const PrepareState &S) {
  const Knobs &K = c->knobs;
  TraceParams &p = L.params;
  const uint64_t numRays = rays_of_apply(c);
  c->numRaysLast = numRays;
  uint64_t first = 0, last = numRays;
  if (c->rayCount) {
    first = std::min(c->rayFirst, numRays);
    last = std::min(numRays, first + c->rayCount);
  }
  c->rayFirstLaunch = first;
  c->rayEndLaunch = last;
  const uint64_t span = last - first;
  c->batchCap = std::max<uint32_t>((uint32_t)std::min<uint64_t>(span, K.batchRays.value_or(1ull << 27)), 1u);
  // (Overlapping the generator of batch b+1 on a second stream with the tracer of batch b was measured slower in every
  //  round — 13.4 against 11.3 ms per C2 step in round 3: both kernels want the same issue slots and smaller batches
  //  sort less coherently — and is gone from the code.)
  // sort bins: far-plane cells holding ~40 rays each, VR_BIN_CAP slots (measured: 64 / 32 -> 128 / 40: generator
  // 5.0 -> 4.75 ms, C2 +2.5 %)
  p.binCap = K.binCap;
  c->raysPerBin = K.raysPerBin;
  // (not on a scene with relief: the rippled plane measured 5 % slower in its tight launch with the aligned grid — its
  //  packets are set by the predicted-hit key and the relief clip, not by the lattice: profiles/aligned_bins_ab.txt)
  L.binAlign = K.binAlign && !L.relief;
  const StreamExtent e = stream_extent(c, L.binAlign, c->batchCap, L.relief, p);
  c->numBins = e.numBins;
  L.binGrid = e.grid;
  // (the loose launch numbers its slots from looseSlotBase on, and bit 31 of such a number marks a spill-queue record)
  if (L.relief && (e.slots >= (1ull << 32) || e.looseSlots >= (1ull << 31)))
    return fail(c, VR_E_STATE, "ray stream too large for 32-bit record slots (relief bins)");
  c->slotStride = e.slots;
  // 32-byte records for every particle (vr_types.hpp); a non-absorbing particle under a source whose origin plane or
  // draw count varies (tilted, grid, host rays) adds 16 bytes per ray in a side array
  // (a stateful model's init draws before the source sample: its draw count varies too)
  L.recExtra = c->src.records_carry_side_array(c->usePrimaryDirection, S.stateful, L.absorb);
  if (L.recExtra)
    VR_HIP(c, c->dRecExtra.ensure_grow((size_t)c->batchCap * 4));
  L.genWeights = c->src.generator_writes_weights();
  if (L.genWeights)
    VR_HIP(c, c->dSurfRayWeights.ensure_grow(c->batchCap));
  if (S.stateful) // (the state of every ray of a batch, float4 per ray; room for vr_reserve_rays' largest batch)
    VR_HIP(c, c->dRayState.ensure_grow((size_t)std::max<uint64_t>(c->batchCap, std::min<uint64_t>(c->reserveRays, 1ull << 27)) * 4));
  size_t slotsWant = e.slots, binsWant = e.cntWords;
  if (c->reserveRays > span) { // vr_reserve_rays: room for the largest apply() announced
    TraceParams q = p;
    const StreamExtent r = stream_extent(c, L.binAlign, (uint32_t)std::min<uint64_t>(c->reserveRays, 1ull << 27), L.relief, q);
    slotsWant = std::max(slotsWant, r.slots);
    binsWant = std::max(binsWant, r.cntWords);
  }
  VR_HIP(c, c->dSlotRec.ensure_grow(slotsWant * 8));
  VR_HIP(c, c->dBinCount.ensure_grow(binsWant));
  return VR_OK;
}

// The kernel of a launch whose traceMode is MODE_ABSORB_FLAT: the ladder of that kernel's variants (vr_types.hpp, modes 8 to
// 12), climbed as far as it goes.  A rung needs the rung below, its knob, the scene's fact and its kernel in the catalogue
// (a run-time model's code object has none of them).  Every other launch: its traceMode
static int absorb_flat_kernel_mode(const vr_context *c, KernelSet set, const ParticleLaunch &L) {
  const Knobs &K = c->knobs;
  const auto exists = [&](int m) { return trace_kernel_exists(set, c->geo.D, c->geo.geo, trace_kernel_particle(L.kernelParticle, m), m); };
  // one normal and one radius for the whole cloud (build_scene: vr_context::uniformDisks)
  if (L.traceMode != MODE_ABSORB_FLAT || !K.uniformDisks || !c->uniformDisks || !exists(MODE_ABSORB_FLAT_UNIFORM))
    return L.traceMode;
  // ... the disks also share a plane normal to a coordinate axis (vr_context::planarDisks)
  if (!K.planarDisks || !c->planarDisks || !exists(MODE_ABSORB_FLAT_PLANAR))
    return MODE_ABSORB_FLAT_UNIFORM;
  // ... that kernel in its one-point-per-round form (vr_planar_disks.hpp (1) - (3))
  if (!K.planarRound || !exists(MODE_ABSORB_FLAT_PLANAR_ROUND))
    return MODE_ABSORB_FLAT_PLANAR;
  // ... with its candidates from the lattice table where the cloud is a lattice cloud (vr_context::planarLattice) whose
  // windows fit a wave (vr_planar_lattice.hpp)
  if (!K.planarLattice || !c->planarLattice ||
      !lattice_window_pays(lattice_reach(c->geo.diskRadius, c->geo.gridDelta, 1e-5f * scene_scale(c)), 1.f / c->geo.gridDelta) ||
      !exists(MODE_ABSORB_FLAT_LATTICE))
    return MODE_ABSORB_FLAT_PLANAR_ROUND;
  // ... each lane testing the four disks at the corners of its point's cell, where no other disk can accept the point
  if (!K.latticeLaneTests || !L.latticeLanesScene || !exists(MODE_ABSORB_FLAT_LATTICE_LANES))
    return MODE_ABSORB_FLAT_LATTICE;
  return MODE_ABSORB_FLAT_LATTICE_LANES;
}

// launch geometry of the persistent kernels: trace mode, the loose launch of a relief scene, blocks per CU
static int choose_trace_mode(vr_context *c, const ParticleSpec &sp, ParticleLaunch &L, const PrepareState &S) {
  const Knobs &K = c->knobs;
  const int D = c->geo.D;
  // (the modes: enum TraceMode, vr_types.hpp)
  // absorbing particles: a (nearly) flat surface is served by packets alone; a structured one
  // ends most rounds in per-lane walks and wants the straggler carry-over (MODE_ABSORB)
  // general particles on a flat surface of disks: the general kernel with the packet query's crediting (MODE_GENERAL_FLAT)
  // (the lean extended kernel P_EXT — data labels, per-material sticking, global data — has the packet query's
  //  crediting too; P_EXT_FULL, the instantiation with the rare options, stays on MODE_GENERAL)
  // "flat": 95 % of the surface shown to the source lies in one plane AND the scene box is thin along the source
  // axis — the packet query clips its rays to that box, and a box half a grid cell thick already lets the few
  // grazing rays of a wave stretch its query over dozens of primitives (a 10^6-disk plane with ONE 50 x 50 bump of
  // 0.3 cells: the absorbing kernel 6.4 -> 8.3 ms, the general one 11 -> 18; the kernels for structured scenes are
  // then 2 - 6 % ahead of the flat ones.  DESIGN.md section 10: a flat layer + relief decomposition would close this)
  // (with flux statistics the lean extended kernel has MODE_GENERAL_FLAT too, but no relief modes: the catalogue,
  //  trace_kernel_exists, vr_types.hpp — what prepare may ask for is what it lists)
  const KernelSet set = sp.userModel >= 0 ? KERNELS_MODULE : KERNELS_LIBRARY;
  const bool generalFlatOk = !L.absorb && trace_kernel_exists(set, D, c->geo.geo, L.kernelParticle, MODE_GENERAL_FLAT);
  L.traceMode = !L.absorb ? ((S.flatScene && generalFlatOk) ? MODE_GENERAL_FLAT : MODE_GENERAL) : (S.flatScene ? MODE_ABSORB_FLAT : MODE_ABSORB);
  L.looseMode = L.traceMode;
  if (L.relief) { // flat with relief: the flat-scene kernels on the tight bins, the structured-scene ones on the loose
    L.traceMode = L.absorb ? MODE_ABSORB_RELIEF : MODE_GENERAL_RELIEF;
    if (!L.absorb && !K.noSpill)
      L.looseMode = MODE_RESUME; // ... which also resume the rays the tight general kernel spills (TraceParams::spillRec)
  }
  if (K.generalFlat.has_value() && generalFlatOk)
    L.traceMode = *K.generalFlat ? MODE_GENERAL_FLAT : MODE_GENERAL;
  if (K.absorbCarry.has_value() && L.absorb)
    L.traceMode = *K.absorbCarry ? MODE_ABSORB : MODE_ABSORB_FLAT;
  if (S.smallScene)
    L.traceMode = MODE_SMALL;
  if (L.traceMode != MODE_ABSORB_RELIEF && L.traceMode != MODE_GENERAL_RELIEF) { // (a switch above took the mode back)
    L.relief = false;
    L.params.reliefCoarse = nullptr;
  }
  // (the rule's verdict on the scene alone: vr_planar_lattice.hpp, "four corners per lane")
  L.latticeLanesScene = c->planarLattice && lattice_lanes_rule(c->geo.diskRadius, c->geo.gridDelta, lattice_lanes_coord(scene_scale(c), c->geo.gridDelta));
  L.kernelMode = absorb_flat_kernel_mode(c, set, L);
  int blocks = 1;
  L.userKernel = nullptr;
  L.userGen = nullptr;
  if (sp.userModel >= 0) { // the kernel of the model's own code object
    UserModel &um = c->userModels[sp.userModel];
    if (L.stats) // (the module's twin with the statistics compiled in: built on first use)
      VR_TRY(ensure_stats_module(c, um));
    const std::map<int, hipFunction_t> &kernels = L.stats ? um.statsKernels : um.kernels; // (find_trace_kernels: the same predicate)
    auto it = kernels.find(module_kernel_key(D, c->geo.geo, L.traceMode));
    if (!trace_kernel_exists(set, D, c->geo.geo, L.kernelParticle, L.traceMode) || it == kernels.end())
      return fail(c, VR_E_STATE, S.stateful ? "stateful particle model: only the general kernels (MODE 0 / 4) carry the state"
                                            : "run-time particle model: no kernel for this geometry / mode in its code object");
    L.userGen = S.stateful ? um.gen[D == 3 ? 1 : 0] : nullptr;
    L.userKernel = it->second;
    int nb = 0;
    if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&nb, L.userKernel, VR_BLOCK, trace_dynamic_lds(L.traceMode, L.params.smallBytes)) != hipSuccess)
      nb = 2;
    blocks = std::max(1, nb);
  } else {
    for (int m : {L.kernelMode, L.relief ? L.looseMode : L.kernelMode}) // (launch_trace would refuse it: said here, by name)
      if (!trace_kernel_exists(set, D, c->geo.geo, trace_kernel_particle(L.kernelParticle, m), m))
        return fail(c, VR_E_STATE, ("no trace kernel for this geometry / particle in MODE " + std::to_string(m)).c_str());
    blocks = std::max(1, trace_blocks_per_cu(D, c->geo.geo, L.kernelParticle, L.kernelMode, L.params.smallBytes));
  }
  // a small launch does better on fewer persistent waves: every wave pays its start-up and its tail.  Best grid on
  // P(100), blocks per CU (tools/small_launch.py): 3 10^5 rays 1, 6 10^5 2, 10^6 3, 2 - 3 10^6 4, 10^7 and more all of
  // them — about sqrt(rays / 10^5).  10^6 rays: 0.69 -> 0.49 ms (absorbing 0.47 -> 0.31)
  if (L.traceMode != MODE_SMALL)
    blocks = std::min(blocks, std::max(1, (int)std::lround(std::sqrt((double)c->batchCap / 1e5))));
  L.grid = (unsigned)c->numCUs * (unsigned)K.traceBlocks.value_or(blocks);
  L.looseGrid = 0;
  if (L.relief) { // (the loose bins hold about a tenth of the rays)
    int lb = std::max(1, trace_blocks_per_cu(D, c->geo.geo, L.kernelParticle, L.looseMode, 0));
    lb = std::min(lb, std::max(1, (int)std::lround(std::sqrt((double)c->batchCap / 1e6))));
    L.looseGrid = (unsigned)c->numCUs * (unsigned)K.looseBlocks.value_or(lb);
  }
  return VR_OK;
}

// The tile buckets of a lattice-lanes launch (vr_tile_buckets.hpp).  Eligible: the launch runs MODE_ABSORB_FLAT_LATTICE_LANES
// in three dimensions with the plain generator of the library (no tilted direction, no side array, no weights, no relief,
// no kernel experiment), the lattice fits VR_TILE_MAX_TILES tiles of the knob's size, and the buckets' record slots —
// behind the overflow region in the same buffer — keep the 32-bit slot index.  Anything else: the
// launch as it was.  (That the launch is alone in its generator group is seen where the groups are made: run_batch.)
static int plan_tile_buckets(vr_context *c, ParticleLaunch &L) {
  const Knobs &K = c->knobs;
  const TraceParams &p = L.params;
  L.tileBuckets = false;
  L.tile = TileParams{};
  if (!K.tileBuckets || L.kernelMode != MODE_ABSORB_FLAT_LATTICE_LANES || c->geo.D != 3 || L.gen != GEN_RANDOM || L.userGen ||
      L.userKernel || L.relief || L.recExtra || L.genWeights || p.useBasis || K.debugFlags != 0u || !c->planarLattice)
    return VR_OK;
  // The source has to look at the FRONT of the disks: the plane normal to the source axis and its normal against the
  // rays.  From behind every hit is a back-face hit, which the tile kernel cannot end — it would hand every ray on, a
  // bucket write, a read and a copy for nothing.  (A ray's component along the source axis is posNeg times a cosine.)
  {
    float n[3];
    std::memcpy(n, c->uniformWords, sizeof(n));
    if (c->planarAxis != p.rayDir || !(p.posNeg * n[c->planarAxis] < 0.f))
      return VR_OK;
  }
  const int shift = std::min(VR_TILE_SHIFT_MAX, std::max(VR_TILE_SHIFT_MIN, K.tileShift));
  const int t1 = lattice_tiles_axis(c->latticeN[0], shift), t2 = lattice_tiles_axis(c->latticeN[1], shift);
  if ((uint64_t)t1 * (uint64_t)t2 > VR_TILE_MAX_TILES)
    return VR_OK;
  L.tile.shift = shift;
  L.tile.tiles1 = t1;
  L.tile.tiles2 = t2;
  L.tile.numTiles = (uint32_t)(t1 * t2);
  L.tileSide = (double)(1 << shift) * (double)c->geo.gridDelta;
  L.tileSrcArea = ((double)p.hi1 - (double)p.lo1) * ((double)p.hi2 - (double)p.lo2);
  // workgroups per bucket: about four blocks per CU in all, so that a launch of few tiles still fills the chip
  // (C2, 256 tiles, trace phase in one call: 2 / 4 / 8 workgroups per bucket 1.58 / 1.63 / 1.99 ms)
  L.tile.slices = std::min<uint32_t>(64u, std::max<uint32_t>(1u, (4u * (uint32_t)c->numCUs + L.tile.numTiles - 1u) / L.tile.numTiles));
  const uint64_t rays = std::max<uint64_t>(c->batchCap, std::min<uint64_t>(c->reserveRays, 1ull << 27));
  const uint64_t cap = K.tileCap.value_or(lattice_tile_capacity(rays, L.tileSide, L.tileSrcArea));
  const uint64_t slots = (uint64_t)c->slotStride + (uint64_t)L.tile.numTiles * cap;
  if (slots >= (1ull << 32))
    return VR_OK;
  VR_HIP(c, c->dSlotRec.ensure_grow((size_t)slots * 8));
  VR_HIP(c, c->dTileCount.ensure_grow(VR_TILE_MAX_TILES));
  // (this context's device: the generator's resident blocks, the tile kernel's dynamic LDS where a tile needs more than
  //  the default limit — asked once per context and tile size)
  if (c->tileGenBlocks == 0)
    c->tileGenBlocks = tile_gen_blocks_per_cu();
  if (lattice_tile_lds_bytes(shift) > 48u * 1024u && shift > c->tileLdsShift) {
    VR_HIP(c, tile_trace_allow_lds(shift));
    c->tileLdsShift = shift;
  }
  L.tileBuckets = true;
  return VR_OK;
}

// the launch's scratch: walk stacks, RNG slabs, the spill queue (buffers every particle of the apply shares)
static int size_scratch(vr_context *c, const ParticleLaunch &L, const PrepareState &S) {
  // deep part of the per-lane walk's stack (entries beyond the LDS-resident ones), one slab per resident wave
  {
    const size_t waves = (size_t)std::max<unsigned>(L.grid, (unsigned)c->numCUs * 8u) * (VR_BLOCK / 64);
    if (waves > c->walkStackWaves) {
      VR_HIP(c, c->dWalkStack.ensure(waves * (size_t)VR_STACK_GLOBAL * 64u));
      c->walkStackWaves = waves;
    }
  }
  // tier-2 RNG slabs (312 x 64 words per resident wave): only a kernel that can draw more than
  // 156 numbers per ray touches them — the general trace kernel and the tilted-source generator
  {
    size_t waves = 0;
    if (!L.absorb)
      waves = (size_t)std::max(L.grid, L.looseGrid) * (VR_BLOCK / 64);
    if (c->src.generator_draws_past_tier1(c->usePrimaryDirection, S.stateful))
      waves = std::max(waves, (size_t)c->numCUs * 8u * (VR_BLOCK / 64)); // launch_gen's grid bound (gen_state_kernel's and gen_user_source_kernel's too)
    if (waves > c->scratchWaves) {
      VR_HIP(c, c->dScratch.ensure(waves * 312u * 64u));
      c->scratchWaves = waves;
    }
  }
  if (L.relief && L.looseMode == MODE_RESUME) { // the spill queue of the tight general relief kernel
    // (a record per ray of a batch + the unused end of every wave's last 64-record block)
    VR_HIP(c, c->dSpillRec.ensure_grow(((size_t)c->batchCap + (size_t)L.grid * (VR_BLOCK / 64) * 64u) * 16));
    VR_HIP(c, c->dSpillCount.ensure(1));
  }
  return VR_OK;
}

// the launch's TraceParams (the shared buffers' addresses: launch_params, at launch time)
static int fill_trace_params(vr_context *c, const ParticleSpec &sp, ParticleLaunch &L, PrepareState &S) {
  const Knobs &K = c->knobs;
  TraceParams &p = L.params;
  const uint32_t N = c->geo.numPrims;
  uint32_t seed = c->runNumber + c->rngSeed; // rayTraceKernel.hpp:100
  if (c->haveSharedSeed) { // (vr_apply_sharded with random seeds: the one seed every rank agreed on)
    seed = c->sharedSeed;
  } else if (c->useRandomSeed) {
    std::random_device rd;
    seed = (uint32_t)rd();
  }
  p.nodes = c->dNodes.p;
  p.qnodes = c->dQNodes.p;
  p.pnodes = c->dPNodes.p;
  p.numNodes = c->numNodes;
  for (int k = 0; k < 3; ++k) {
    p.qbase[k] = c->qbase[k];
    p.qscale[k] = c->qscale[k];
  }
  p.prims = c->dPrims.p;
  p.wide = c->haveWide ? c->dWide.p : nullptr;
  p.wideTopFirst = c->wideRoot[0];
  p.wideTopCount = c->wideRoot[1];
  p.widePrimBase = c->wideRoot[2];
  p.pqMaxFrontier = K.pqFrontier;
  p.pqMaxCand = K.pqCand;
  for (int k = 0; k < 3; ++k) {
    p.sceneLo[k] = c->sceneLo[k];
    p.sceneHi[k] = c->sceneHi[k];
  }
  p.nbDist = 2 * c->geo.diskRadius;
  p.geoD = c->geo.D;
  p.pqPad = 1e-5f * scene_scale(c); // >> the rounding of the clip (1e-7 relative); the boxes carry their own 4e-6 pad
  p.nbOff = c->dNbOff.p;
  p.nbIds = c->dNbIds.p;
  { // wall table + scalar frame: one slot per particle of the apply (each kernel stages its own launch's frame in LDS)
    const size_t nSlots = c->launches.size();
    if (c->dWalls.cap < nSlots * VR_WALL_TABLE)
      VR_HIP(c, c->dWalls.ensure(nSlots * VR_WALL_TABLE));
    if (c->frameHostAll.size() < nSlots * VR_WALL_TABLE)
      c->frameHostAll.assign(nSlots * VR_WALL_TABLE, 0.f);
  }
  p.wallTable = c->dWalls.p + (size_t)L.slot * VR_WALL_TABLE;
  p.planeStride = c->accStride * c->accReplicas;
  p.accStride = c->accStride;
  p.numData = sp.numData;
  p.particleKind = sp.kernelKind;
  p.meanFreePath = sp.meanFreePath;
  std::memcpy(p.particleParams, sp.params, sizeof(p.particleParams));
  p.globalVec = (c->globalStride && !c->globalVecs.empty()) ? c->dGlobalVec.p : nullptr;
  p.globalScalars = c->globalScalars.empty() ? nullptr : c->dGlobalScalars.p;
  p.numGlobalVec = p.globalVec ? (uint32_t)c->globalVecs.size() : 0u;
  p.globalStride = c->globalStride;
  p.numGlobalScalars = (uint32_t)c->globalScalars.size();
  p.useWdist = c->useWdist ? 1 : 0;
  // the source fields: every pointer of a kind that is not in force is null
  p.gridPoints = nullptr;
  p.gridCount = 0;
  p.eeGrid = 2.f / (sp.sourcePower + 1); // raySourceGrid.hpp:22
  p.hostOrg = p.hostDir = nullptr;
  p.hostDraws = nullptr;
  p.hostWeights = nullptr;
  p.surfPos = p.surfNrm = p.surfWeights = nullptr;
  p.surfRays = 0;
  p.surfOffset = 0.f;
  L.source = SourceCtx{};
  L.gen = c->src.generator(c->usePrimaryDirection);
  const RaySource &src = c->src;
  switch (src.kind) {
  case SourceKind::Random: break;
  case SourceKind::Grid:
    p.gridPoints = c->dGrid.p;
    p.gridCount = (uint32_t)(src.gridPoints.size() / 3);
    break;
  case SourceKind::HostRays:
    p.hostOrg = c->dHostOrg.p;
    p.hostDir = c->dHostDir.p;
    p.hostDraws = src.hostDraws.empty() ? nullptr : c->dHostDraws.p;
    p.hostWeights = src.hostWeights.empty() ? nullptr : c->dHostWeights.p;
    break;
  case SourceKind::Surface: // (hostWeights: the batch's start weights, written by the generator — batch_params)
    p.surfPos = c->dSurfPos.p;
    p.surfNrm = c->dSurfNrm.p;
    p.surfWeights = c->dSurfWeights.p;
    p.surfRays = (uint32_t)RaySource::rays_per_surface_point(c->numRaysPerPoint, c->numRaysFixed);
    p.surfOffset = src.surfOffset;
    break;
  case SourceKind::Model: { // the generator of the model's code object, records without / with the RNG cursors, and what
                            // it sees (its table's address as it is now: a later setter clears `prepared`)
    L.userGen = c->sourceModels[src.sourceModel].gen[c->geo.D == 3 ? 1 : 0][L.absorb ? 0 : 1];
    SourceCtx &sc = L.source;
    for (int k = 0; k < 3; ++k) {
      sc.bbLo[k] = c->bbLo[k];
      sc.bbHi[k] = c->bbHi[k];
    }
    sc.srcCoord = c->ts[3] ? c->bbHi[c->ts[0]] : c->bbLo[c->ts[0]];
    sc.rayDir = c->ts[0];
    sc.firstDir = c->ts[1];
    sc.secondDir = c->ts[2];
    sc.posNeg = (float)c->ts[4];
    sc.gridDelta = c->geo.gridDelta;
    sc.sourcePower = sp.sourcePower;
    sc.tableCount = src.srcTableCount;
    sc.table = src.srcTableCount ? c->dSrcTable.p : nullptr;
    std::memcpy(sc.params, src.srcParams, sizeof(sc.params));
    break;
  }
  }
  p.accMask = c->accReplicas - 1u;
  VR_HIP(c, c->dCounters.ensure(C_BLOCK * c->launches.size()));
  VR_HIP(c, c->dWorkQ.ensure(VR_QUEUES * VR_QUEUE_STRIDE));
  p.numQueues = VR_QUEUES;
  // a stateful model: its state buffer and the material ids of its hooks (the caller's id of the original primitive) go
  // into the launch frame (VR_F_STATE_*, VR_F_MAT_*).  (Both are sized by what every particle of an apply shares — rays
  // per batch, primitives — so a later particle's prepare does not move them.)
  S.dMaterial = nullptr;
  if (S.stateful && (c->materialOnDevice || !c->materialIds.empty())) { // (a device copy, zeros behind the ids given)
    VR_TRY(ensure_device_material_ids(c));
    const uint32_t given = std::min(N, c->materialCount);
    VR_HIP(c, c->dPrimMaterial.ensure(N));
    if (given)
      VR_HIP(c, hipMemcpyAsync(c->dPrimMaterial.p, c->dMaterialIds.p, (size_t)given * 4, hipMemcpyDeviceToDevice, c->stream));
    if (N > given)
      VR_HIP(c, hipMemsetAsync(c->dPrimMaterial.p + given, 0, (size_t)(N - given) * 4, c->stream));
    S.dMaterial = c->dPrimMaterial.p;
  }
  // the packet query's search margin (frontier reuse over neighbouring rounds, flat-scene kernels): in units of the
  // neighbourhood distance 2 r (disks) / 1.7 grid cells (triangles); pqMaxFrontier <= 24 entries fit the cached lists
  p.pqMargin = K.pqMargin * (c->geo.geo == 0 ? 2.f * c->geo.diskRadius : 1.7f * c->geo.gridDelta);
  p.idxList = nullptr;
  p.batchFirst = c->rayFirstLaunch;
  p.batchCount = 0;
  p.ovCap = c->batchCap;
  p.numBins = c->numBins;
  p.seed = seed;
  p.numPrims = N;
  p.maxReflections = c->maxReflections;
  p.maxBoundaryHits = c->maxBoundaryHits;
  p.chunk = 64;
  p.rayDir = c->ts[0];
  p.firstDir = c->ts[1];
  p.secondDir = c->ts[2];
  p.minMax = c->ts[3];
  p.posNeg = (float)c->ts[4];
  p.ee = 1.f / (sp.sourcePower + 1); // raySourceRandom.hpp:21
  p.sticking = sp.sticking;
  p.bc0 = c->boundaryConds[0];
  p.bc1 = c->boundaryConds[1];
  p.useBasis = c->usePrimaryDirection ? 1 : 0;
  if (c->usePrimaryDirection)
    host_orthonormal_basis(c->primaryDirection, p.basis);
  else
    std::memset(p.basis, 0, sizeof(p.basis));
  p.srcCoord = c->ts[3] ? c->bbHi[c->ts[0]] : c->bbLo[c->ts[0]];
  p.lo1 = c->bbLo[c->ts[1]];
  p.hi1 = c->bbHi[c->ts[1]];
  p.lo2 = c->bbLo[c->ts[2]];
  p.hi2 = c->bbHi[c->ts[2]];
  {
    const float lr = c->bbLo[c->ts[0]], hr = c->bbHi[c->ts[0]];
    float scale = 0.f;
    for (int k = 0; k < 3; ++k)
      scale = std::max(scale, std::max(std::fabs(c->bbLo[k]), std::fabs(c->bbHi[k])));
    const float margin = 1e-3f * std::max(scale, hr - lr) + 1e-6f;
    p.wallLoR = lr - margin;
    p.wallHiR = hr + margin;
  }
  p.keyCoord = K.keyCoord.value_or(c->keyCoord);
  p.invExt1 = (p.hi1 > p.lo1) ? 1.f / (p.hi1 - p.lo1) : 0.f;
  p.invExt2 = (p.hi2 > p.lo2) ? 1.f / (p.hi2 - p.lo2) : 0.f;
  p.packetBudget = K.packetBudget;
  // (share of parked lanes at which the pending leaves are tested: sweep 10 / 18 / 25 / 35 / 50 — disks flat between
  //  18 and 35; triangles, whose leaf test is the longer one, 10: trenchMesh 0.1 28.3 -> 27.5 ms, C4 20.6 -> 20.2)
  p.walkPark = K.walkPark.value_or(c->geo.geo == 1 ? 10u : 25u);
  p.walkExit = K.walkExit; // (sweep 12 .. 36: 12 - 20 within 1 %, 36 slower by 4 - 7 %)
  p.packetRatio = K.packetRatio;
  p.debugFlags = K.debugFlags;
  return VR_OK;
}

// height field over the source plane: for particles that go on after a hit ("segments that rise clear", vr_trace_kernel.hpp)
static int build_height_field(vr_context *c, const ParticleLaunch &L, PrepareState &S) {
  S.heightField = !L.absorb && c->geo.numPrims && !c->knobs.noHeightField;
  if (!S.heightField)
    return VR_OK;
  const bool stale = c->hfBuild != c->bvhBuilds || c->hfAxes[0] != c->ts[0] || c->hfAxes[1] != c->ts[1] ||
                     c->hfAxes[2] != c->ts[2] || c->hfAxes[3] != c->ts[3];
  if (!stale)
    return VR_OK;
  const int D = c->geo.D;
  HeightFieldParams &q = c->hf;
  q.prims = c->dPrims.p;
  q.n = c->geo.numPrims;
  q.geo = c->geo.geo;
  q.ax = c->ts[0];
  q.a1 = c->ts[1];
  q.a2 = c->ts[2];
  q.sign = c->ts[3] ? 1.f : -1.f; // (ts[3]: the source plane lies at the max side)
  const float ext1 = c->sceneHi[q.a1] - c->sceneLo[q.a1], ext2 = D == 3 ? c->sceneHi[q.a2] - c->sceneLo[q.a2] : 0.f;
  // (tile side in grid cells; sweep 2 / 3 / 4 / 6 / 8: see DESIGN.md 7)
  float tile = std::max(c->knobs.hfTile * c->geo.gridDelta, std::max(ext1, ext2) / 256.f);
  if (!(tile > 0.f))
    tile = 1.f;
  q.lo1 = c->sceneLo[q.a1];
  q.lo2 = D == 3 ? c->sceneLo[q.a2] : 0.f;
  q.invTile = 1.f / tile;
  q.nx = std::max(1, std::min(256, (int)std::ceil(ext1 / tile)));
  q.ny = D == 3 ? std::max(1, std::min(256, (int)std::ceil(ext2 / tile))) : 1;
  q.pad = 8e-7f * scene_scale(c); // (a dozen ulp of the largest coordinate: see DESIGN.md 5.2)
  VR_HIP(c, c->dHfRaw.ensure((size_t)q.nx * q.ny));
  VR_HIP(c, c->dHf.ensure((size_t)q.nx * q.ny));
  q.raw = c->dHfRaw.p;
  q.field = c->dHf.p;
  VR_HIP(c, launch_height_field(q, c->stream));
  c->hfBuild = c->bvhBuilds;
  for (int k = 0; k < 4; ++k)
    c->hfAxes[k] = c->ts[k];
  return VR_OK;
}

// the launch's wall table and scalar frame (VR_F_*, vr_frame.hpp), staged in LDS by the trace kernels
static int write_launch_frame(vr_context *c, const ParticleLaunch &L, const PrepareState &S) {
  const TraceParams &p = L.params;
  float *const f = c->frameHostAll.data() + (size_t)L.slot * VR_WALL_TABLE;
  std::memcpy(f, c->wallsHost, sizeof(c->wallsHost));
  std::fill(f + 96, f + VR_WALL_TABLE, 0.f); // (VR_F_EXTRA_*, the records' side-array address: the kernel writes it)
  auto bits = [](int32_t v) {
    float r;
    std::memcpy(&r, &v, 4);
    return r;
  };
  auto addr = [&](int lo, const void *ptr) { // a device address as two words
    const uint64_t a = (uint64_t)(uintptr_t)ptr;
    f[lo] = bits((int32_t)(uint32_t)(a & 0xFFFFFFFFull));
    f[lo + 1] = bits((int32_t)(uint32_t)(a >> 32));
  };
  f[VR_F_SRC_PLANE] = p.srcCoord;
  f[VR_F_RAYDIR] = bits(p.rayDir);
  f[VR_F_FIRSTDIR] = bits(p.firstDir);
  f[VR_F_SECONDDIR] = bits(p.secondDir);
  f[VR_F_LO1] = p.lo1;
  f[VR_F_LO1 + 1] = p.hi1;
  f[VR_F_LO1 + 2] = p.lo2;
  f[VR_F_LO1 + 3] = p.hi2;
  f[VR_F_WALL_LO_R] = p.wallLoR;
  f[VR_F_WALL_HI_R] = p.wallHiR;
  for (int k = 0; k < 3; ++k) {
    f[VR_F_SCENE_LO + k] = p.sceneLo[k];
    f[VR_F_SCENE_HI + k] = p.sceneHi[k];
  }
  f[VR_F_PQ_PAD] = p.pqPad;
  f[VR_F_BC0] = bits(p.bc0);
  f[VR_F_BC1] = bits(p.bc1);
  f[VR_F_NB_DIST] = p.nbDist;
  if (S.heightField) { // (build_height_field)
    const HeightFieldParams &q = c->hf;
    f[VR_F_HF_LO1] = q.lo1;
    f[VR_F_HF_LO2] = q.lo2;
    f[VR_F_HF_INVT] = q.invTile;
    f[VR_F_HF_TILE] = 1.f / q.invTile;
    f[VR_F_HF_TOP] = (q.sign > 0.f ? c->sceneHi[q.ax] : -c->sceneLo[q.ax]); // above this nothing is left (the BVH's root box)
    f[VR_F_HF_SIGN] = q.sign;
    f[VR_F_HF_NX] = bits(q.nx);
    f[VR_F_HF_NY] = bits(q.ny);
    addr(VR_F_HF_PTR_LO, q.field);
  }
  const ModeTraits kernel = mode_traits(L.kernelMode); // (the launch's kernel: which blocks of the frame it reads)
  if (kernel.uniform) { // (an absorbing launch: no height field, whose first words these are — vr_frame.hpp, VR_F_UD_*)
    if (S.heightField)
      return fail(c, VR_E_STATE, "a launch with uniform disks has no height field: their frame words are the same");
    float w[4];
    std::memcpy(w, c->uniformWords, sizeof(w));
    for (int k = 0; k < 3; ++k)
      f[VR_F_UD_N + k] = w[k];
    f[VR_F_UD_RADIUS] = w[3];
    f[VR_F_UD_T] = uniform_disk_threshold(w[3]);
    if (kernel.planar) { // (VR_F_PD_*: the next words of the same block)
      f[VR_F_PD_AXIS] = bits(c->planarAxis);
      f[VR_F_PD_COORD] = bits((int32_t)c->planarWord);
    }
    if (kernel.planarRound) { // (VR_F_PR_*: words of the height field and of the relief field, which such a launch has not)
      if (L.relief)
        return fail(c, VR_E_STATE, "a planar-round launch has no relief field: their frame words are the same");
      float ca;
      std::memcpy(&ca, &c->planarWord, 4);
      f[VR_F_PR_QLO] = ca - p.pqPad;
      f[VR_F_PR_QHI] = ca + p.pqPad;
      planar_wall_inner(p.lo1, p.hi1, f[VR_F_PR_IN], f[VR_F_PR_IN + 1]);
      planar_wall_inner(p.lo2, p.hi2, f[VR_F_PR_IN + 2], f[VR_F_PR_IN + 3]);
      int b1, b2;
      planar_in_plane_axes(c->planarAxis, b1, b2);
      f[VR_F_PR_SB] = p.sceneLo[b1] - p.pqPad;
      f[VR_F_PR_SB + 1] = p.sceneHi[b1] + p.pqPad;
      f[VR_F_PR_SB + 2] = p.sceneLo[b2] - p.pqPad;
      f[VR_F_PR_SB + 3] = p.sceneHi[b2] + p.pqPad;
    }
    if (kernel.lattice) { // (VR_F_PL_*: words of a stateful model and of the data log, which such a launch has not)
      if (S.stateful || S.logs)
        return fail(c, VR_E_STATE, "a planar-lattice launch has no stateful model: their frame words are the same");
      addr(VR_F_PL_PTR_LO, c->dLattice.p);
      f[VR_F_PL_N1] = bits(c->latticeN[0]);
      f[VR_F_PL_N2] = bits(c->latticeN[1]);
      f[VR_F_PL_PHASE1] = c->latticePhase[0];
      f[VR_F_PL_PHASE2] = c->latticePhase[1];
      f[VR_F_PL_INVD] = 1.f / c->geo.gridDelta;
      f[VR_F_PL_REACH] = lattice_reach(w[3], c->geo.gridDelta, p.pqPad);
    }
  }
  if (L.relief) { // the relief field's fine tiles (relief_clip, vr_packet_query.hpp)
    const ReliefParams &q = c->rf;
    f[VR_F_RF_LO1] = q.lo1;
    f[VR_F_RF_LO2] = q.lo2;
    f[VR_F_RF_INVT] = q.invTile;
    f[VR_F_RF_TILE] = q.tile;
    f[VR_F_RF_NX] = bits(q.nx);
    f[VR_F_RF_NY] = bits(q.ny);
    addr(VR_F_RF_PTR_LO, q.fine);
  }
  if (S.stateful) {
    addr(VR_F_STATE_LO, c->dRayState.p);
    addr(VR_F_MAT_LO, S.dMaterial);
  }
  if (S.logs) {
    addr(VR_F_LOG_LO, c->dDataLog.p);
    addr(VR_F_LOGCTL_LO, c->dDataLog.p + c->logTotal);
  }
  VR_HIP(c, hipMemcpyAsync(c->dWalls.p + (size_t)L.slot * VR_WALL_TABLE, f, VR_WALL_TABLE * 4, hipMemcpyHostToDevice, c->stream));
  return VR_OK;
}

// everything the launch of particle `sp` needs (scene build and areas only when they changed), into L.  Every device call
// goes to c->stream in this order.
static int prepare_one(vr_context *c, const ParticleSpec &sp, ParticleLaunch &L) {
  VR_HIP(c, hipSetDevice(c->device));
  const auto t0 = std::chrono::steady_clock::now();
  c->castValid = false; // (a prepare that fails half way leaves nothing for vr_cast_rays* to read)
  const bool redoConfig = c->configDirty || c->geometryDirty;
  if (redoConfig)
    VR_TRY(setup_source_frame(c));
  // the BVH's child order follows the source side: a new source direction rebuilds it
  if (c->builtOrderAxis != c->ts[0] || c->builtOrderSign != (c->ts[3] ? 1.f : -1.f))
    c->geometryDirty = true;
  if (c->geometryDirty) {
    VR_TRY(build_scene(c));
    c->geometryDirty = false;
    ++c->bvhBuilds;
    c->builtOrderAxis = c->ts[0];
    c->builtOrderSign = c->ts[3] ? 1.f : -1.f;
  }
  if (redoConfig || !c->areasValid)
    VR_TRY(compute_areas(c));
  // (the sticking map: one particle keeps its own from apply to apply; the particles of a list are prepared in turn, each time)
  if (redoConfig || c->particleDirty || c->specs.size() > 1)
    VR_TRY(prepare_sticking(c, sp, L));
  c->configDirty = false;
  c->particleDirty = false;
  if (c->globalDirty)
    VR_TRY(upload_global_data(c));
  PrepareState S;
  VR_TRY(choose_particle_kernel(c, sp, L, S));
  VR_TRY(build_relief_field(c, sp, L, S));
  VR_TRY(ensure_accumulators(c));
  if (c->src.sourceDirty)
    VR_TRY(upload_source_data(c));
  VR_TRY(size_ray_stream(c, L, S));
  VR_TRY(choose_trace_mode(c, sp, L, S)); // (after the ray stream: blocks follow the batch size; the buffers keep the relief layout)
  VR_TRY(size_scratch(c, L, S));
  VR_TRY(fill_trace_params(c, sp, L, S));
  VR_TRY(plan_tile_buckets(c, L));
  VR_TRY(build_height_field(c, L, S));
  VR_TRY(write_launch_frame(c, L, S));
  c->castParams = L.params; // what vr_cast_rays* reads of this prepare (vr_cast_rays.cpp)
  c->castBuild = c->bvhBuilds;
  c->castValid = true;
  const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (redoConfig)
    c->buildSeconds = secs; // a cheap re-prepare (new seed / ray range only) keeps the last build time
  c->prepared = true;
  c->launched = false;
  c->haveResult = false;
  return VR_OK;
}

// The data log of the apply (vr_set_data_log_shape): every stateful model of the particle list with a log_data hook adds to
// the one log (the reference keeps one dataLog_ per Trace).  Checks the shape against the hooks, sizes the buffer and
// uploads the control words behind the sums; the sums themselves are zeroed when the apply launches.
static int prepare_data_log(vr_context *c) {
  c->logActive = false;
  if (c->logRowSizes.empty())
    return VR_OK;
  int hooks = 0, rowsNeeded = 0;
  for (const ParticleSpec &sp : c->specs)
    if (sp.userModel >= 0 && c->userModels[sp.userModel].logRows > 0) {
      ++hooks;
      rowsNeeded = std::max(rowsNeeded, c->userModels[sp.userModel].logRows);
    }
  if (!hooks)
    return fail(c, VR_E_INVALID, "a data-log shape is set (vr_set_data_log_shape) but no particle model of this apply has a "
                                 "log_data hook (kLogRows == 0): nothing would fill the log; clear the shape or use a "
                                 "stateful model that logs");
  if ((int)c->logRowSizes.size() < rowsNeeded)
    return fail(c, VR_E_INVALID, ("the data-log shape has " + std::to_string(c->logRowSizes.size()) + " rows, the particle "
                                  "model's log_data hook writes " + std::to_string(rowsNeeded) + " (kLogRows): too few rows").c_str());
  VR_HIP(c, hipSetDevice(c->device));
  VR_HIP(c, c->dDataLog.ensure((size_t)c->logTotal + VR_LOG_CTL_WORDS));
  std::vector<unsigned long long> &h = c->logCtlHost;
  h.assign(VR_LOG_CTL_WORDS, 0ull);
  h[VR_LOG_ROWS] = c->logRowSizes.size();
  h[VR_LOG_HEADROOM] = rank_headroom(c->worldSize);
  h[VR_LOG_FLAGS] = c->knobs.logPlainAtomics ? 1ull : 0ull;
  unsigned long long off = 0;
  for (size_t r = 0; r < c->logRowSizes.size(); ++r) {
    h[VR_LOG_OFFSETS + r] = off;
    off += c->logRowSizes[r];
  }
  h[VR_LOG_OFFSETS + c->logRowSizes.size()] = off;
  VR_HIP(c, hipMemcpyAsync(c->dDataLog.p + c->logTotal, h.data(), h.size() * 8, hipMemcpyHostToDevice, c->stream));
  c->logActive = true;
  return VR_OK;
}

} // namespace vr

extern "C" {

// Trace::apply() set-up: every particle (vr_set_particles) is prepared in turn — its kernel variant, launch geometry,
// per-material sticking, accumulator planes and counter block — with ONE seed for the whole apply
// (gpu/raygTrace.hpp:163-248).  The knobs are read here, once per apply.
int vr_apply_prepare(vr_context *c) {
  if (!c)
    return VR_E_INVALID;
  c->knobs = read_knobs();
  const size_t nPart = c->numParticles();
  if (nPart > 1 && c->useRandomSeed && !c->haveSharedSeed) { // one draw for all particles of this apply
    std::random_device rd;
    c->sharedSeed = (uint32_t)rd();
    c->haveSharedSeed = true;
    c->keepSharedSeed = false;
  }
  if (c->launches.size() != nPart) {
    c->launches.clear();
    c->launches.resize(nPart);
  }
  VR_TRY(prepare_data_log(c));
  VR_TRY(check_settings(c)); // (refuses an empty particle list: behind it specs.size() == nPart)
  uint32_t base = 0;
  for (size_t q = 0; q < c->specs.size(); ++q) {
    ParticleLaunch &L = c->launches[q];
    L.slot = (uint32_t)q;
    L.dataBase = base;
    VR_TRY(prepare_one(c, c->specs[q], L));
    base += c->specs[q].numData + (c->fluxStats ? (uint32_t)VR_STAT_PLANES : 0u);
  }
  return VR_OK;
}

} // extern "C"
