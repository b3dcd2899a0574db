// vr_trace.hip — the HIP kernels of the flux tracer (gfx950).
//
// The reference traces rays one by one in index order (rayTraceKernel.hpp:118).
// Ray i's whole random stream is a pure function of (i, seed), so any order
// gives the same flux; the GPU path is therefore organised as an HBM-resident
// RAY STREAM, processed in batches:
//
//   gen_kernel      one lane per ray index: per-ray mt19937_64 (lazy, streaming),
//                   power-cosine source sample -> 32-byte ray record (+ the 16-byte
//                   RNG cursors when the particle keeps going after a hit), written
//                   DIRECTLY into the sort bin of the cell where the ray crosses the
//                   sort plane (bin cursor = one atomic; no separate sort pass), so a
//                   wavefront's 64 rays end in the same neighbourhood: their BVH node
//                   / primitive fetches are wave-uniform (scalar loads) and their
//                   traversal loops stay converged.
//   trace_kernel    persistent wavefronts pull bins; a lane whose ray ends pulls
//                   the next one (wave-wide compaction by ballot + prefix
//                   popcount), so bounce chains of different length do not idle
//                   the wave.  Per segment: closest hit (wave-uniform packet query /
//                   packet traversal, per-lane ordered walk with its stack in LDS as
//                   the fallback; then the boundary walls), then the reference's
//                   state machine (rayTraceKernel.hpp:155-335).
//
// Where what lives (all in this directory):
//   vr_generate.hpp      source sampling, sort keys, record store, the surface sampler; the library's generators
//   vr_trace_kernel.hpp  the trace kernel, its helpers and its tuning knobs (the modes: enum TraceMode, vr_types.hpp)
//   vr_modules.hpp       the two run-time module sections: a source model's generator; a particle model's trace kernels
//                        and stateful generator
//   vr_kernel_table.hpp  the catalogue's trace kernels (trace_kernel_exists, vr_types.hpp) as a table: lookup, launcher, occupancy
//   vr_trace.hip         this file: the library's generators and its statistics-off trace kernels, or — compiled as a
//                        run-time module (VR_USER_MODULE, vr_models.cpp) — the module section
//   vr_trace_stats.hip   the library's trace kernels with flux statistics compiled in: the same table over their two ids
//   vr_diag.hip          the diagnostic kernels of the vr_debug_* entry points
//   vr_bvh.hip           scene build: LBVH, 64-ary box tree, neighbourhood CSR, bvh_check
//   vr_sort.hip          the radix sort of the build and the exclusive scan
//   vr_fields.hip        height field and relief field over the source plane (every prepare)
//   vr_ingest.hip        device-resident inputs: disks, meshes, sort-plane histogram, global data, sticking, surface source
//   vr_post.hip          the results stage: smoothing, areas, flux gather, normalisation, statistics
//   vr_map.hip           per-primitive values at the caller's points: a range / nearest walk of the resident BVH
//   vr_setup_common.hpp  private to those six: the ordered-uint trick
//   vr_cast.hip          closest-hit queries for the caller's rays: the pair walk and the walls, segment after segment
//   vr_cast.hpp          ... the per-ray bookkeeping of that kernel, plain C++ (the host compiler takes it alone)
// A run-time module is compiled from this file and what it includes: the Makefile's MODEL_SRCS names those files once.
#include <hip/hip_runtime.h>

#ifdef VR_USER_MODULE
#include "vr_modules.hpp"
#else
#include "vr_generate.hpp"
#include "vr_kernel_table.hpp"
#include "vr_tile_buckets.hpp"

namespace vr {

// ---------------------------------------------------------------------------
// host-callable launchers
// ---------------------------------------------------------------------------

// source: one of the library's five generators (enum Generator, vr_types.hpp)
static StreamKernel gen_kernel_for(Generator source, int D, bool keepRng, bool relief) {
  const int v = (D == 2 ? 0 : 2) + (keepRng ? 1 : 0); // 2-D / 3-D, records without / with the RNG cursors
  if (source == GEN_RANDOM && relief) { // the plain generator on a scene with relief: predicted-hit key, loose bins
    static const StreamKernel reliefGen[4] = {gen_kernel<2, false, true>, gen_kernel<2, true, true>, gen_kernel<3, false, true>,
                                              gen_kernel<3, true, true>};
    return reliefGen[v];
  }
#define VR_GEN(DD, KEEP)                                                                                               \
  {gen_kernel<DD, KEEP, false>, gen_basis_kernel<DD, KEEP>, gen_grid_kernel<DD, KEEP>, gen_host_kernel<DD, KEEP>,      \
   gen_surface_kernel<DD, KEEP>}
  static const StreamKernel gen[4][5] = {VR_GEN(2, false), VR_GEN(2, true), VR_GEN(3, false), VR_GEN(3, true)};
#undef VR_GEN
  return gen[v][source];
}

hipError_t launch_gen(const TraceParams &p, Generator gen, int D, bool keepRng, unsigned maxBlocks, hipStream_t s) {
  if (gen < GEN_RANDOM || gen > GEN_SURFACE) // (a source model's generator is its module's: not in the table)
    return hipErrorInvalidValue;
  unsigned grid = (p.batchCount + VR_BLOCK - 1) / VR_BLOCK;
  if (grid == 0)
    return hipSuccess;
  if (grid > maxBlocks)
    grid = maxBlocks; // grid-stride; bounds the tier-2 slabs to grid waves
  hipLaunchKernelGGL(gen_kernel_for(gen, D, keepRng, p.reliefCoarse && p.binCount), dim3(grid), dim3(VR_BLOCK), 0, s, p);
  return hipGetLastError();
}

// The trace kernel of a launch: the statistics-off particle ids of the catalogue (0 DiffuseParticle, 1 SpecularParticle,
// P_EXT, P_EXT_FULL; the two statistics ids: vr_trace_stats.hip's table).  mode: a TraceMode
using LibraryKernels = TraceKernelTable<0, P_EXT_FULL>;

hipError_t launch_trace(const TraceParams &p, int D, int geo, int particle, int mode, unsigned grid,
                        hipStream_t s) {
  if (particle >= P_EXT_STATS)
    return launch_trace_stats(p, D, geo, particle, mode, grid, s);
  return LibraryKernels::launch(p, D, geo, particle, mode, grid, s);
}

// The tile-bucket pipeline of a lattice-lanes launch (vr_tile_buckets.hpp): the generator that files the simple rays by
// lattice tile, and the kernel that finishes them against a tile held in LDS.
// Block of 256 threads, chunk of 1 024 rays: 29 KB of LDS, five blocks per CU.  (Measured in one call on C2, generator:
// 256 / 1024 4.16 ms, 512 / 2048 4.31, 256 / 2048 4.73, 1024 / 4096 4.78; with 32-cell tiles 4.49 against 5.32 for 512 /
// 2048: profiles/tile_buckets_ab.txt.)
using TileGen = void (*)(const TraceParams, const TileParams);
constexpr unsigned VR_TILE_GEN_BLOCK = 256, VR_TILE_GEN_CHUNK = 1024;
static const TileGen tileGen = gen_tile_kernel<VR_TILE_GEN_BLOCK, VR_TILE_GEN_CHUNK>;

// resident blocks per CU of the tile generator on the current device (the caller keeps the answer with its context)
int tile_gen_blocks_per_cu() {
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, tileGen, VR_TILE_GEN_BLOCK, 0) != hipSuccess || nb < 1)
    nb = 1;
  return nb;
}
// (the grid is what the chip holds at once: a block more per CU would run as a second wave of blocks behind the first)
hipError_t launch_gen_tiles(const TraceParams &p, const TileParams &tp, unsigned maxBlocks, hipStream_t s) {
  if (tp.numTiles == 0u || tp.numTiles > VR_TILE_MAX_TILES || tp.shift < VR_TILE_SHIFT_MIN || tp.shift > VR_TILE_SHIFT_MAX || maxBlocks == 0u)
    return hipErrorInvalidValue;
  unsigned grid = (p.batchCount + VR_TILE_GEN_CHUNK - 1) / VR_TILE_GEN_CHUNK;
  if (grid == 0)
    return hipSuccess;
  if (grid > maxBlocks)
    grid = maxBlocks;
  hipLaunchKernelGGL(tileGen, dim3(grid), dim3(VR_TILE_GEN_BLOCK), 0, s, p, tp);
  return hipGetLastError();
}

// the tile kernel's dynamic LDS for tiles of 2^shift cells a side allowed on the current device (above the default limit
// it has to be asked for, per device: the caller does so when it prepares a launch)
hipError_t tile_trace_allow_lds(int shift) {
  if (shift < VR_TILE_SHIFT_MIN || shift > VR_TILE_SHIFT_MAX)
    return hipErrorInvalidValue;
  return hipFuncSetAttribute(reinterpret_cast<const void *>(tile_trace_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)lattice_tile_lds_bytes(shift));
}
hipError_t launch_tile_trace(const TraceParams &p, const TileParams &tp, hipStream_t s) {
  if (tp.numTiles == 0u || tp.numTiles > VR_TILE_MAX_TILES || tp.slices == 0u || tp.shift < VR_TILE_SHIFT_MIN || tp.shift > VR_TILE_SHIFT_MAX)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(tile_trace_kernel, dim3(tp.numTiles * tp.slices), dim3(VR_TILE_TRACE_BLOCK), lattice_tile_lds_bytes(tp.shift), s, p, tp);
  return hipGetLastError();
}

int trace_blocks_per_cu(int D, int geo, int particle, int mode, unsigned smallBytes) {
  if (particle >= P_EXT_STATS)
    return trace_stats_blocks_per_cu(D, geo, particle, mode, smallBytes);
  return LibraryKernels::blocks_per_cu(D, geo, particle, mode, smallBytes);
}

} // namespace vr
#endif // VR_USER_MODULE
