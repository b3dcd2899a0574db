// vr_kernel_table.hpp — the catalogue's trace kernels (trace_kernel_exists, vr_types.hpp) as a table, and the one lookup,
// launcher and occupancy query over it.  Private to vr_trace.hip and vr_trace_stats.hip, which each hold a range of
// particle ids, and to vr_modules.hpp, whose table is what instantiates a module's kernels.
#pragma once
#include <array>
#include <utility>

#include "vr_kernels.hpp"
#include "vr_trace_kernel.hpp"

namespace vr {

// every generator and every trace kernel: a kernel over the launch's TraceParams
using StreamKernel = void (*)(const TraceParams);

// The kernels of particle ids P_LO .. P_HI, indexed [(((D - 2) * 2 + geo) * particles + particle - P_LO) * VR_NUM_MODES + mode];
// nullptr where the catalogue has none.  An entry that exists is what instantiates its kernel.
template <int P_LO, int P_HI> struct TraceKernelTable {
  static constexpr int particles = P_HI - P_LO + 1, size = 4 * particles * VR_NUM_MODES;
  template <int I> static constexpr StreamKernel entry() {
    constexpr int mode = I % VR_NUM_MODES, particle = P_LO + I / VR_NUM_MODES % particles, dg = I / VR_NUM_MODES / particles;
    if constexpr (trace_kernel_exists(VR_KERNEL_SET, 2 + dg / 2, dg % 2, particle, mode))
      return trace_kernel<2 + dg / 2, dg % 2, particle, mode>;
    else
      return nullptr;
  }
  template <int... I> static constexpr std::array<StreamKernel, size> make(std::integer_sequence<int, I...>) { return {entry<I>()...}; }
  static constexpr std::array<StreamKernel, size> kernels = make(std::make_integer_sequence<int, size>{});

  // the kernel that serves a request (an absorbing mode: particle id 0, trace_kernel_particle), or nullptr
  static StreamKernel find(int D, int geo, int particle, int mode) {
    particle = trace_kernel_particle(particle, mode);
    if (particle < P_LO || particle > P_HI || !trace_kernel_exists(VR_KERNEL_SET, D, geo, particle, mode))
      return nullptr;
    return kernels[(((D - 2) * 2 + geo) * particles + particle - P_LO) * VR_NUM_MODES + mode];
  }
  // a request without a kernel is an error, never another kernel
  static hipError_t launch(const TraceParams &p, int D, int geo, int particle, int mode, unsigned grid, hipStream_t s) {
    const StreamKernel k = find(D, geo, particle, mode);
    if (!k)
      return hipErrorInvalidDeviceFunction;
    hipLaunchKernelGGL(k, dim3(grid), dim3(VR_BLOCK), trace_dynamic_lds(mode, p.smallBytes), s, p);
    return hipGetLastError();
  }
  static int blocks_per_cu(int D, int geo, int particle, int mode, unsigned smallBytes) {
    const StreamKernel k = find(D, geo, particle, mode);
    int nb = 0;
    if (!k || hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k, VR_BLOCK, trace_dynamic_lds(mode, smallBytes)) != hipSuccess)
      return 2;
    return nb;
  }
};

} // namespace vr
