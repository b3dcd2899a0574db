// vr_trace_stats.hip — the library's trace kernels with FLUX STATISTICS compiled in (vr_set_flux_statistics; the template
// ids P_EXT_STATS / P_EXT_FULL_STATS of vr_types.hpp, STATS in vr_trace_kernel.hpp) and their launchers.
//
// A translation unit of its own: the table of vr_trace.hip — what a statistics-off launch picks — holds exactly the
// kernels it held before.  A statistics-on launch that is not absorbing runs one of these, whatever its particle: the
// built-in DiffuseParticle / SpecularParticle as models 0 / 1 of the registry (the same arithmetic as their own
// instantiations: the same flux and counters).  They exist for MODE_GENERAL and MODE_SMALL (any geometry) and, the lean
// one on disks, MODE_GENERAL_FLAT; a scene with relief is traced by MODE_GENERAL.
#include <hip/hip_runtime.h>

#include "vr_kernels.hpp"
#include "vr_trace_kernel.hpp"

namespace vr {

using StreamKernel = void (*)(const TraceParams);

template <int D, int GEO> static StreamKernel stats_kernel_of(bool full, int mode) {
  if (full)
    return mode == MODE_SMALL ? trace_kernel<D, GEO, P_EXT_FULL_STATS, MODE_SMALL> : trace_kernel<D, GEO, P_EXT_FULL_STATS, MODE_GENERAL>;
  if (mode == MODE_SMALL)
    return trace_kernel<D, GEO, P_EXT_STATS, MODE_SMALL>;
  if constexpr (GEO == 0) {
    if (mode == MODE_GENERAL_FLAT)
      return trace_kernel<D, 0, P_EXT_STATS, MODE_GENERAL_FLAT>;
  }
  return trace_kernel<D, GEO, P_EXT_STATS, MODE_GENERAL>;
}

// particle: P_EXT_STATS or P_EXT_FULL_STATS; mode: MODE_GENERAL, MODE_SMALL or (lean, disks) MODE_GENERAL_FLAT — anything
// else has no kernel here, and a missing kernel is an error
static StreamKernel stats_kernel_for(int D, int geo, int particle, int mode) {
  const bool full = particle == P_EXT_FULL_STATS;
  if (particle != P_EXT_STATS && !full)
    return nullptr;
  if (mode != MODE_GENERAL && mode != MODE_SMALL && !(mode == MODE_GENERAL_FLAT && geo == 0 && !full))
    return nullptr;
  if (D == 2)
    return geo ? stats_kernel_of<2, 1>(full, mode) : stats_kernel_of<2, 0>(full, mode);
  return geo ? stats_kernel_of<3, 1>(full, mode) : stats_kernel_of<3, 0>(full, mode);
}

hipError_t launch_trace_stats(const TraceParams &p, int D, int geo, int particle, int mode, unsigned grid, hipStream_t s) {
  const StreamKernel k = stats_kernel_for(D, geo, particle, mode);
  if (!k)
    return hipErrorInvalidDeviceFunction;
  hipLaunchKernelGGL(k, dim3(grid), dim3(VR_BLOCK), mode == MODE_SMALL ? p.smallBytes : 0, s, p);
  return hipGetLastError();
}

int trace_stats_blocks_per_cu(int D, int geo, int particle, int mode, unsigned smallBytes) {
  const StreamKernel k = stats_kernel_for(D, geo, particle, mode);
  int nb = 0;
  if (!k || hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k, VR_BLOCK, mode == MODE_SMALL ? smallBytes : 0) != hipSuccess)
    return 2;
  return nb;
}

} // namespace vr
