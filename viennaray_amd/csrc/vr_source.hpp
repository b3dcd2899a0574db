// vr_source.hpp — the ray source in force: ONE of five kinds, the host-side payload of that kind, the one transition
// every source setter ends in, and the questions the stages of an apply ask about the source.  Host code without a HIP
// header (tests/aux/source_state.cpp compiles it alone); the entry points are in vr_source.cpp.  The device buffers of
// the sources (dGrid, dHost*, dSurf*, dSrcTable, dSurfRayWeights) are members of the context: they are HIP objects, and
// they are kept across switches on purpose (a simulation that alternates between two sources re-allocates nothing).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "vr_types.hpp"

namespace vr {

// (SourceRandom with a primary direction is a configuration of Random — vr_set_primary_direction, independent of every
//  source setter — not a kind: the questions below that depend on it take it as `primary`)
enum class SourceKind { Random, Grid, HostRays, Surface, Model };

struct RaySource {
  SourceKind kind = SourceKind::Random;
  // Grid: SourceGrid origins (raySourceGrid.hpp)
  std::vector<float> gridPoints;
  // HostRays: the rays of a host-side Source callback
  std::vector<float> hostOrg, hostDir;
  std::vector<uint32_t> hostDraws; // engine outputs each ray's callback consumed (empty: none)
  std::vector<float> hostWeights;  // Source::getInitialRayWeight(idx) (empty: 1)
  // Surface (vr_set_surface_source): the tables live on the device, uploaded when they are set
  uint32_t surfCount = 0;          // source points
  float surfArea = 0.f, surfOffset = 0.f;
  // Model (vr_set_source_model): sampled on the device by its own generator; the table lives on the device
  int32_t sourceModel = -1;        // index of the model in vr_context::sourceModels
  bool srcHasWeight = false;       // ... and its VrUserSource::kHasWeight
  float srcParams[VR_SOURCE_PARAMS] = {0};
  uint32_t srcTableCount = 0;
  uint64_t srcNumRays = 0;         // its own ray count (0: SourceRandom's)
  bool sourceDirty = false;        // dGrid / dHost* may not hold gridPoints / host* yet (upload_source_data)

  // ---- the transition ---------------------------------------------------------------------------------------------
  // Every setter ends here, with the payload of `k` already written and nothing left that can fail (the rule of
  // commit_geometry: a setter does everything that can fail first, so a refused call leaves the previous source in
  // force).  This is the one place that drops the payload of the other kinds: the vectors, and the two scalars that say
  // "none" (surfCount, sourceModel); the other scalars of a kind not in force keep their last values, which nothing reads.
  void become(SourceKind k) {
    if (k != SourceKind::Grid)
      gridPoints.clear();
    if (k != SourceKind::HostRays) {
      hostOrg.clear();
      hostDir.clear();
      hostDraws.clear();
      hostWeights.clear();
    }
    if (k != SourceKind::Surface)
      surfCount = 0;
    if (k != SourceKind::Model)
      sourceModel = -1;
    kind = k;
  }

  // ---- the setters' host side -----------------------------------------------------------------------------------------
  // The calls that go back to SourceRandom are of two kinds.  Source in force after the call, by the one before it:
  //   call                                      Random     Grid       HostRays   Surface    Model
  //   vr_set_source_grid(NULL, 0)               Random     Random     Random     Random     Random      clear-always
  //   vr_set_host_rays(.., 0)                   Random     Random     Random     Random     Random      clear-always
  //   vr_set_surface_source(n = 0) (+ _device)  unchanged  unchanged  unchanged  Random     unchanged   clear-if Surface
  //   vr_set_source_model(-1)                   unchanged  unchanged  unchanged  unchanged  Random      clear-if Model
  // The first two are Trace::resetSource() and a host source of no rays: whatever the source was, it is gone.  The last
  // two are clearSurfaceSource() and setSource(nullptr) of a façade that keeps these sources apart from the others: they
  // take back only what their own setter set.  "unchanged" also leaves `prepared` as it is: clear_if says whether it
  // changed anything.
  void clear_always() { become(SourceKind::Random); }
  bool clear_if(SourceKind k) {
    if (kind != k)
      return false;
    become(SourceKind::Random);
    return true;
  }
  // (sourceDirty is raised by every call of the three setters whose payload comes up from the host, the clearing ones
  //  included: upload_source_data then finds nothing to upload)
  void set_grid(const float *points3, uint32_t n) { // n == 0: clear-always
    sourceDirty = true;
    if (n == 0)
      return clear_always();
    gridPoints.assign(points3, points3 + (size_t)n * 3);
    become(SourceKind::Grid);
  }
  void set_host_rays(const float *org3, const float *dir3, const uint32_t *draws, uint64_t n) { // n == 0: clear-always
    sourceDirty = true;
    if (n == 0)
      return clear_always();
    hostOrg.assign(org3, org3 + (size_t)n * 3);
    hostDir.assign(dir3, dir3 + (size_t)n * 3);
    if (draws)
      hostDraws.assign(draws, draws + (size_t)n);
    else
      hostDraws.clear();
    hostWeights.clear(); // (the weights belonged to the rays before)
    become(SourceKind::HostRays);
  }
  // one weight per host ray, or none (n == 0: all 1); false: refused, nothing changed.  While host rays are not in force
  // their count is 0: every n > 0 is refused.
  bool set_host_weights(const float *weights, uint64_t n) {
    if (n && n != hostOrg.size() / 3)
      return false;
    hostWeights.assign(weights, weights + (size_t)n);
    sourceDirty = true;
    return true;
  }
  void set_surface(uint32_t n, float sourceArea, float sourceOffset) { // (n > 0: the tables are on the device)
    surfCount = n;
    surfArea = sourceArea;
    surfOffset = sourceOffset;
    become(SourceKind::Surface);
  }
  void set_model(int32_t id, bool hasWeight, const float *params, uint32_t nparams, uint32_t tableCount, uint64_t numRays) {
    sourceModel = id;
    srcHasWeight = hasWeight;
    std::fill(std::copy(params, params + nparams, srcParams), srcParams + VR_SOURCE_PARAMS, 0.f);
    srcTableCount = tableCount;
    srcNumRays = numRays;
    become(SourceKind::Model);
  }

  // ---- the questions the stages ask ---------------------------------------------------------------------------------
  // rays per point of a surface source (gpu/raygTrace.hpp:134-149: the fixed count, if set, is the launch's x extent)
  static uint64_t rays_per_surface_point(uint64_t perPoint, uint64_t fixed) { return fixed ? fixed : perPoint; }

  // The ray count of an apply.  rayTraceKernel.hpp:57-61: numRaysFixed, or source.getNumPoints() * numRaysPerPoint —
  // SourceRandom: the geometry's points; SourceGrid: the grid's; host rays: exactly those given (the fixed count does not
  // apply); a surface source: rays per point on every point; a model: its own count if it has one, else SourceRandom's.
  uint64_t rays_of_apply(uint32_t numPrims, uint64_t perPoint, uint64_t fixed) const {
    uint64_t points = numPrims;
    switch (kind) {
    case SourceKind::Surface: return (uint64_t)surfCount * rays_per_surface_point(perPoint, fixed);
    case SourceKind::HostRays: return hostOrg.size() / 3;
    case SourceKind::Model:
      if (srcNumRays)
        return srcNumRays;
      break;
    case SourceKind::Grid: points = gridPoints.size() / 3; break;
    case SourceKind::Random: break;
    }
    return fixed == 0 ? points * perPoint : fixed;
  }

  // The rays start with weights of their own: host rays that were given weights, a surface source (the point's weight),
  // a model with kHasWeight.  The absorbing kernels credit unit weights, so there is no absorbing kernel then.
  bool rays_start_weighted() const {
    return (kind == SourceKind::HostRays && !hostWeights.empty()) || generator_writes_weights();
  }
  // The GENERATOR writes the start weights of a batch (dSurfRayWeights, addressed like a host source's): the surface
  // source and a model with kHasWeight.  Host rays are not among them: their weights come up from the host, once.
  bool generator_writes_weights() const {
    return kind == SourceKind::Surface || (kind == SourceKind::Model && srcHasWeight);
  }
  // The origin plane or the draw count varies from ray to ray, so the 32-byte records of a particle that goes on after a
  // hit cannot leave them out: they carry the side array (TraceParams::recExtra).  Everything but the plain SourceRandom
  // — tilted: its rejection loop; grid, host rays, surface, model: any origin — and every source under a stateful
  // particle model, whose init draws before the source sample.  An absorbing launch reads neither.
  bool records_carry_side_array(bool primary, bool stateful, bool absorb) const {
    return !absorb && (primary || kind != SourceKind::Random || stateful);
  }
  // The generator can draw past tier 1 of the engine (156 outputs per ray), so the RNG slabs are sized for the generator
  // grid: the tilted SourceRandom (a rejection loop), host rays (a callback may have consumed any number of outputs, which
  // the generator skips), a model (any code), a stateful particle model's init.  NOT the grid and the surface source,
  // which are among the side-array sources above: their samples are a fixed handful of draws (grid: the direction;
  // surface: two), far below 156.  (With a primary direction set, a grid or surface launch still gets the slabs: the
  // flag is asked, not the generator — more memory than needed, never less.)
  bool generator_draws_past_tier1(bool primary, bool stateful) const {
    return primary || kind == SourceKind::HostRays || kind == SourceKind::Model || stateful;
  }
  // The plain source that relief packets need: the generator predicts a ray's first hit from an origin on the source
  // plane and a cosine direction about the axis (bin_of_relief) — SourceRandom without a primary direction, nothing else.
  bool is_plain(bool primary) const { return kind == SourceKind::Random && !primary; }
  // A stateful particle model runs its init on the device before the source sample, in its module's own generator, which
  // samples SourceRandom (plain or tilted): no other source.
  bool admits_stateful_model() const { return kind == SourceKind::Random; }
  // The library's generator of a launch (a model's is its module's own: GEN_SOURCE_MODEL)
  Generator generator(bool primary) const {
    switch (kind) {
    case SourceKind::Grid: return GEN_GRID;
    case SourceKind::HostRays: return GEN_HOST;
    case SourceKind::Surface: return GEN_SURFACE;
    case SourceKind::Model: return GEN_SOURCE_MODEL;
    case SourceKind::Random: break;
    }
    return primary ? GEN_BASIS : GEN_RANDOM;
  }
};

} // namespace vr
