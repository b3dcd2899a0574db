// vr_radiosity.hip — the iteration of solveRadiosity over a recorded link table (vr_radiosity_solve_device;
// include/viennaray_amd.h has the definition, vr_radiosity.hpp the arithmetic and the table's index, vr_radiosity_solve.cpp
// the host side; the table itself is written by vr_gather.hip's gather_samples_kernel<GEO, D, true>).  A translation unit
// of its own: nothing an apply() runs is in it, and nothing here walks, draws a random number or keeps a stack.
//
//   radiosity_rho_kernel      the caller's reflectivity (by original id, or one scalar) into leaf order, and the lowest
//                             index that fails radiosity_rho_ok into one word.
//   radiosity_init_kernel     F_0 from the direct sums, e_1 = rho F_0.
//   radiosity_iterate_kernel  one iteration: a block of RAD_SPLIT waves owns 64 leaf slots, lane = slot; wave w streams the
//                             link rows of samples w, w + RAD_SPLIT, ... (one 256-byte line per row and wave) and gathers
//                             e[link] from the leaf-ordered emission table, where neighbouring lanes read neighbouring
//                             entries; the waves' int64 partial sums meet in LDS (exact: any order gives the same bits);
//                             wave 0 writes F_t and e_{t+1} and folds |F_t - F_{t-1}| into the iteration's word with
//                             one integer atomicMax per wave.  A kernel whose predecessor's word already meets the
//                             tolerance returns at once, so a batch of launches stops where one at a time would.
//   radiosity_unpermute_kernel, radiosity_orig_of_leaf_kernel, radiosity_debug_links_kernel: leaf order <-> original ids.
#include <hip/hip_runtime.h>

#include "vr_kernels.hpp"
#include "vr_radiosity.hpp"

namespace vr {

constexpr unsigned RAD_SPLIT = 4;   // waves of a block, each with every RAD_SPLIT-th sample of the block's 64 slots
constexpr unsigned RAD_UNROLL = 4;  // link loads of a lane in flight before the first dependent gather

__global__ void radiosity_rho_kernel(const float *rho, float scalar, const unsigned *leafOfOrig, unsigned n, float *rhoLeaf,
                                     unsigned *bad) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const float r = rho ? rho[i] : scalar;
  if (!radiosity_rho_ok(r))
    atomicMin(bad, i);
  rhoLeaf[leafOfOrig[i]] = r; // (leafOfOrig is a permutation of 0 .. n - 1)
}

__global__ void radiosity_init_kernel(const unsigned long long *direct, const float *rhoLeaf, unsigned n, unsigned samples,
                                      float *F, float *e) {
  const unsigned q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n)
    return;
  const float f = radiosity_row_result((long long)direct[q], 0, samples);
  F[q] = f;
  e[q] = radiosity_emission(rhoLeaf[q], f);
}

template <bool NT> __device__ __forceinline__ int radiosity_load_link(const int *p) {
  return NT ? __builtin_nontemporal_load(p) : *p;
}

template <bool NT> __global__ __launch_bounds__(64 * RAD_SPLIT) void radiosity_iterate_kernel(const RadiosityArgs a) {
  if (a.prevResidual && radiosity_stops(*a.prevResidual, a.tolerance))
    return; // (the whole grid alike: the solve ended with the iteration before)
  __shared__ long long part[RAD_SPLIT - 1][64];
  const unsigned lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  const unsigned slot = blockIdx.x * 64u + lane; // (the grid has slots / 64 blocks: slot < a.slots <= 2^32)
  const bool valid = slot < a.n;
  long long sum = 0;
  if (valid) {
    // rows w, w + RAD_SPLIT, ...: entry radiosity_link_index(a.slots, slot, k) < a.slots x a.samples for k < a.samples
    unsigned k = w;
    for (; (unsigned long long)k + (RAD_UNROLL - 1u) * RAD_SPLIT < a.samples; k += RAD_UNROLL * RAD_SPLIT) {
      int l[RAD_UNROLL];
#pragma unroll
      for (unsigned u = 0; u < RAD_UNROLL; ++u)
        l[u] = radiosity_load_link<NT>(a.links + radiosity_link_index(a.slots, slot, k + u * RAD_SPLIT));
#pragma unroll
      for (unsigned u = 0; u < RAD_UNROLL; ++u)
        sum += radiosity_link_q(l[u], a.eIn, a.wmax); // (a link is -1 or a leaf position < a.n)
    }
    for (; k < a.samples; k += RAD_SPLIT)
      sum += radiosity_link_q(radiosity_load_link<NT>(a.links + radiosity_link_index(a.slots, slot, k)), a.eIn, a.wmax);
  }
  if (w)
    part[w - 1u][lane] = sum;
  __syncthreads();
  if (w)
    return;
  unsigned r = 0u;
  if (valid) {
#pragma unroll
    for (unsigned v = 0; v + 1u < RAD_SPLIT; ++v)
      sum += part[v][lane];
    const float f = radiosity_row_result((long long)a.direct[slot], sum, a.samples);
    r = radiosity_residual_bits(f, a.F[slot]);
    a.F[slot] = f;
    a.eOut[slot] = radiosity_emission(a.rho[slot], f);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned o = (unsigned)__shfl_xor((int)r, off, 64);
    r = o > r ? o : r;
  }
  if (lane == 0u && r)
    atomicMax(a.residual, r);
}

__global__ void radiosity_unpermute_kernel(const float *F, const unsigned *leafOfOrig, unsigned n, float *out) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n)
    out[i] = F[leafOfOrig[i]];
}

__global__ void radiosity_orig_of_leaf_kernel(const unsigned *leafOfOrig, unsigned n, unsigned *origOfLeaf) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n)
    origOfLeaf[leafOfOrig[i]] = i;
}

// links first .. first + count - 1 of ORIGINAL primitive `prim`, as ORIGINAL ids
__global__ void radiosity_debug_links_kernel(const int *links, unsigned long long slots, const unsigned *leafOfOrig, unsigned prim,
                                             unsigned first, unsigned count, const unsigned *origOfLeaf, int *out) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count)
    return;
  const int l = links[radiosity_link_index(slots, leafOfOrig[prim], first + i)];
  out[i] = l >= 0 ? (int)origOfLeaf[l] : RADIOSITY_NO_LINK;
}

static dim3 blocks_of(unsigned n) { return dim3((n + 255u) / 256u); }

hipError_t launch_radiosity_rho(const float *rho, float scalar, const unsigned *leafOfOrig, unsigned n, float *rhoLeaf,
                                unsigned *bad, hipStream_t st) {
  hipLaunchKernelGGL(radiosity_rho_kernel, blocks_of(n), dim3(256), 0, st, rho, scalar, leafOfOrig, n, rhoLeaf, bad);
  return hipGetLastError();
}
hipError_t launch_radiosity_init(const unsigned long long *direct, const float *rhoLeaf, unsigned n, unsigned samples, float *F,
                                 float *e, hipStream_t st) {
  hipLaunchKernelGGL(radiosity_init_kernel, blocks_of(n), dim3(256), 0, st, direct, rhoLeaf, n, samples, F, e);
  return hipGetLastError();
}
hipError_t launch_radiosity_iterate(const RadiosityArgs &a, bool nontemporal, hipStream_t st) {
  if (a.n == 0 || a.slots < a.n || a.slots % 64u || a.slots > 0x100000000ull)
    return hipErrorInvalidValue;
  const dim3 g((unsigned)(a.slots / 64u)), b(64u * RAD_SPLIT);
  if (nontemporal)
    hipLaunchKernelGGL(radiosity_iterate_kernel<true>, g, b, 0, st, a);
  else
    hipLaunchKernelGGL(radiosity_iterate_kernel<false>, g, b, 0, st, a);
  return hipGetLastError();
}
hipError_t launch_radiosity_unpermute(const float *F, const unsigned *leafOfOrig, unsigned n, float *out, hipStream_t st) {
  hipLaunchKernelGGL(radiosity_unpermute_kernel, blocks_of(n), dim3(256), 0, st, F, leafOfOrig, n, out);
  return hipGetLastError();
}
hipError_t launch_radiosity_orig_of_leaf(const unsigned *leafOfOrig, unsigned n, unsigned *origOfLeaf, hipStream_t st) {
  hipLaunchKernelGGL(radiosity_orig_of_leaf_kernel, blocks_of(n), dim3(256), 0, st, leafOfOrig, n, origOfLeaf);
  return hipGetLastError();
}
hipError_t launch_radiosity_debug_links(const int *links, unsigned long long slots, const unsigned *leafOfOrig, unsigned prim,
                                        unsigned first, unsigned count, const unsigned *origOfLeaf, int *out, hipStream_t st) {
  if (count == 0)
    return hipSuccess;
  hipLaunchKernelGGL(radiosity_debug_links_kernel, blocks_of(count), dim3(256), 0, st, links, slots, leafOfOrig, prim, first,
                     count, origOfLeaf, out);
  return hipGetLastError();
}

} // namespace vr
