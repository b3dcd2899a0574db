// vr_trace_stats.hip — the library's trace kernels with FLUX STATISTICS compiled in (vr_set_flux_statistics; the template
// ids P_EXT_STATS / P_EXT_FULL_STATS of vr_types.hpp, STATS in vr_trace_kernel.hpp) and their launchers.
//
// A translation unit of its own: the table of vr_trace.hip — what a statistics-off launch picks — holds exactly the
// kernels it held before.  A statistics-on launch that is not absorbing runs one of these, whatever its particle: the
// built-in DiffuseParticle / SpecularParticle as models 0 / 1 of the registry (the same arithmetic as their own
// instantiations: the same flux and counters).  Which exist: the catalogue (trace_kernel_exists, vr_types.hpp) — the
// general and the LDS-resident kernel and, the lean one on disks, MODE_GENERAL_FLAT; a scene with relief is traced by
// MODE_GENERAL.
#include <hip/hip_runtime.h>

#include "vr_kernel_table.hpp"

namespace vr {

using StatsKernels = TraceKernelTable<P_EXT_STATS, P_EXT_FULL_STATS>;

hipError_t launch_trace_stats(const TraceParams &p, int D, int geo, int particle, int mode, unsigned grid, hipStream_t s) {
  return StatsKernels::launch(p, D, geo, particle, mode, grid, s);
}

int trace_stats_blocks_per_cu(int D, int geo, int particle, int mode, unsigned smallBytes) {
  return StatsKernels::blocks_per_cu(D, geo, particle, mode, smallBytes);
}

} // namespace vr
