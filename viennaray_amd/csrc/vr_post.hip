// vr_post.hip — the results stage: flux smoothing over the resident neighbourhood, exposed disk areas, accumulators to
// flux, normalisation, the flux statistics and the gather into the caller's primitive order.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "vr_kernels.hpp"
#include "vr_setup_common.hpp"
#include "vr_types.hpp"

namespace vr {

// smoothFlux (rayTraceDisk.hpp:146-193) on the device neighbourhood: weighted average over the
// neighbours whose normal points the same way, weights = normal dot products.  The sum runs
// over the neighbours in ASCENDING ORIGINAL ID like the host path (float addition is ordered),
// so both give the same bits: each thread sorts its (short) list first.  A list longer than the
// local buffer raises *overflow and the host path takes over.
constexpr unsigned SMOOTH_MAX = 48;
__global__ void smooth_flux_kernel(const float *fluxIn, float *fluxOut, const float *normal3, const uint32_t *nbOff,
                                   const uint32_t *nbIds, const uint32_t *order, const uint32_t *leafOfOrig,
                                   unsigned n, unsigned *overflow) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const unsigned q = leafOfOrig[i];
  const unsigned b = nbOff[q], e = nbOff[q + 1];
  if (e - b > SMOOTH_MAX) {
    atomicAdd(overflow, 1u);
    fluxOut[i] = fluxIn[i];
    return;
  }
  unsigned ids[SMOOTH_MAX];
  unsigned cnt = 0;
  for (unsigned j = b; j < e; ++j) { // insertion sort by original id
    const unsigned o = order[nbIds[j]];
    unsigned k = cnt++;
    while (k > 0 && ids[k - 1] > o) {
      ids[k] = ids[k - 1];
      --k;
    }
    ids[k] = o;
  }
  const float nx = normal3[3 * (size_t)i], ny = normal3[3 * (size_t)i + 1], nz = normal3[3 * (size_t)i + 2];
  float vv = fluxIn[i], sum = 1.f;
  for (unsigned k = 0; k < cnt; ++k) {
    const unsigned o = ids[k];
    const float w = (nx * normal3[3 * (size_t)o] + ny * normal3[3 * (size_t)o + 1]) + nz * normal3[3 * (size_t)o + 2];
    if (w > 0.f) {
      vv += fluxIn[o] * w;
      sum += w;
    }
  }
  fluxOut[i] = vv / sum;
}

// smoothFlux(flux, k > 1) (rayTraceDisk.hpp:146-193: a PointNeighborhood of radius k * 2 r, built for the call): the
// neighbourhood is not stored — every thread runs the range query of nb_kernel with the wider radius over the resident
// BVH, keeps the ids it finds (ascending original id, like the host path: float addition is ordered) and averages.
constexpr unsigned SMOOTH_WIDE_MAX = 128;
__global__ void smooth_wide_kernel(const float *fluxIn, float *fluxOut, const float *normal3, SetupParams s, float dist,
                                   unsigned *overflow) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= s.n)
    return;
  const float4 *nodes = reinterpret_cast<const float4 *>(s.nodes);
  const float px = s.points3[3 * (size_t)i], py = s.points3[3 * (size_t)i + 1], pz = s.points3[3 * (size_t)i + 2];
  const float dist2 = dist * dist;
  const float qlo[3] = {px - dist, py - dist, s.D == 2 ? -FLT_MAX : pz - dist};
  const float qhi[3] = {px + dist, py + dist, s.D == 2 ? FLT_MAX : pz + dist};
  unsigned ids[SMOOTH_WIDE_MAX];
  unsigned cnt = 0;
  bool over = false;
  unsigned node = 0;
  while (node != VR_END) {
    const float4 a = nodes[2 * (size_t)node], b = nodes[2 * (size_t)node + 1];
    const unsigned link = __float_as_uint(a.w), esc = __float_as_uint(b.w);
    // (the boxes are the discs' boxes: a disc's box contains its centre, and every centre within `dist` lies in the query box)
    const bool hit = a.x <= qhi[0] && b.x >= qlo[0] && a.y <= qhi[1] && b.y >= qlo[1] && a.z <= qhi[2] && b.z >= qlo[2];
    if (hit && (link & VR_LEAF)) {
      const unsigned first = link & VR_LEAF_FIRST_MASK, num = (link >> 27) & 15u;
      for (unsigned k = 0; k < num; ++k) {
        const unsigned o = s.order[first + k];
        if (o == i)
          continue;
        const float dx = px - s.points3[3 * (size_t)o], dy = py - s.points3[3 * (size_t)o + 1],
                    dz = pz - s.points3[3 * (size_t)o + 2];
        bool near = fabsf(dx) <= dist && fabsf(dy) <= dist && (s.D == 2 || fabsf(dz) <= dist);
        near = near && ((dx * dx + dy * dy) + dz * dz) <= dist2;
        if (!near)
          continue;
        if (cnt == SMOOTH_WIDE_MAX) {
          over = true;
          continue;
        }
        unsigned k2 = cnt++;
        while (k2 > 0 && ids[k2 - 1] > o) { // insertion sort by original id
          ids[k2] = ids[k2 - 1];
          --k2;
        }
        ids[k2] = o;
      }
      node = esc;
    } else {
      node = hit ? link : esc;
    }
  }
  if (over) {
    atomicAdd(overflow, 1u);
    fluxOut[i] = fluxIn[i];
    return;
  }
  const float nx = normal3[3 * (size_t)i], ny = normal3[3 * (size_t)i + 1], nz = normal3[3 * (size_t)i + 2];
  float vv = fluxIn[i], sum = 1.f;
  for (unsigned k = 0; k < cnt; ++k) {
    const unsigned o = ids[k];
    const float w = (nx * normal3[3 * (size_t)o] + ny * normal3[3 * (size_t)o + 1]) + nz * normal3[3 * (size_t)o + 2];
    if (w > 0.f) {
      vv += fluxIn[o] * w;
      sum += w;
    }
  }
  fluxOut[i] = vv / sum;
}

hipError_t launch_smooth_wide(const float *fluxIn, float *fluxOut, const float *normal3, const SetupParams &s, float dist,
                              unsigned *overflow, hipStream_t st) {
  if (s.n == 0)
    return hipSuccess;
  hipLaunchKernelGGL(smooth_wide_kernel, dim3((s.n + 127) / 128), dim3(128), 0, st, fluxIn, fluxOut, normal3, s, dist, overflow);
  return hipGetLastError();
}

hipError_t launch_smooth_flux(const float *fluxIn, float *fluxOut, const float *normal3, const uint32_t *nbOff,
                              const uint32_t *nbIds, const uint32_t *order, const uint32_t *leafOfOrig, unsigned n,
                              unsigned *overflow, hipStream_t st) {
  if (n == 0)
    return hipSuccess;
  hipLaunchKernelGGL(smooth_flux_kernel, dim3((n + 127) / 128), dim3(128), 0, st, fluxIn, fluxOut, normal3, nbOff, nbIds,
                     order, leafOfOrig, n, overflow);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Post-processing on the device: exposed disk areas
// (computeDiskAreas + DiskBoundingBoxXYIntersector, vr_area.hpp) and normalizeFlux
// (rayTraceDisk.hpp:103-142, rayTraceTriangle.hpp:92-130; the reference's own GPU path:
// gpu/kernels/normKernels.cu:58-74).  One thread per primitive, caller's order.
// ---------------------------------------------------------------------------
__global__ void disk_areas_kernel(const float *disk4, const float *normal3, unsigned n, AreaParams p, float *out) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const float4 d = reinterpret_cast<const float4 *>(disk4)[i];
  const float disk[4] = {d.x, d.y, d.z, d.w};
  const float nrm[3] = {normal3[3 * (size_t)i], normal3[3 * (size_t)i + 1], normal3[3 * (size_t)i + 2]};
  out[i] = disk_exposed_area(p, disk, nrm);
}

hipError_t launch_disk_areas(const float *disk4, const float *normal3, unsigned n, const AreaParams &p, float *out,
                             hipStream_t st) {
  if (n == 0)
    return hipSuccess;
  hipLaunchKernelGGL(disk_areas_kernel, dim3((n + 127) / 128), dim3(128), 0, st, disk4, normal3, n, p, out);
  return hipGetLastError();
}

// raw flux as the reference's float vector: float(acc * 2^-40) (acc: int64 fixed point)
__global__ void flux_from_acc_kernel(const unsigned long long *acc, unsigned n, float *flux) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n)
    flux[i] = (float)((double)acc[i] * 9.094947017729282379150390625e-13); // 2^-40
}

// std::max_element over the flux (ordered-uint atomicMax; NaNs never win a `<` in the reference either)
__global__ void flux_max_kernel(const float *flux, unsigned n, unsigned *maxOrd) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  float v = i < n ? flux[i] : -FLT_MAX;
  if (!(v == v))
    v = -FLT_MAX;
  for (int off = 32; off > 0; off >>= 1)
    v = fmaxf(v, __shfl_down(v, off, 64));
  __shared__ float red[4];
  if ((threadIdx.x & 63) == 0)
    red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0)
    atomicMax(maxOrd, f2ord(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]))));
}

// SOURCE: flux *= normFactor / area (all float).  MAX, disks: flux *= (pi r^2 / area) / max in
// double like the reference's `totalDiskArea` (a double); triangles: flux /= max * area (float).
template <int NORM, int GEO>
__global__ void normalize_flux_kernel(float *flux, const float *area, unsigned n, float normFactor, double totalDiskArea,
                                      const unsigned *maxOrd) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  if (NORM == 0) {
    flux[i] *= normFactor / area[i];
  } else {
    const float maxv = ord2f(*maxOrd);
    if (GEO == 0)
      flux[i] = (float)((double)flux[i] * ((totalDiskArea / (double)area[i]) / (double)maxv));
    else
      flux[i] /= maxv * area[i];
  }
}

hipError_t launch_flux_from_acc(const unsigned long long *acc, unsigned n, float *flux, hipStream_t st) {
  if (n == 0)
    return hipSuccess;
  hipLaunchKernelGGL(flux_from_acc_kernel, dim3((n + 255) / 256), dim3(256), 0, st, acc, n, flux);
  return hipGetLastError();
}

// ---- flux statistics (vr_set_flux_statistics) ----
// An absorbing launch credits unit weights only: every credit adds 2^40 to the flux plane, 1 * 1 * 2^40 to the sum of
// squares and 1 to the hit count — the companion planes follow from the flux plane, and its kernels stay as they are.
__global__ void stats_fill_absorbing_kernel(const unsigned long long *flux, unsigned n, unsigned long long *sumsq,
                                            unsigned long long *hits) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const unsigned long long f = flux[i];
    sumsq[i] = f;
    hits[i] = f >> 40;
  }
}

// The per-credit estimator of the Monte-Carlo error of a raw flux sum S1 = sum w over N rays: sigma^2 = sum w^2 - S1^2 / N
// (N x the sample variance of a ray's contribution, the rays that miss counted as zeros).  KIND 1: sigma in raw flux
// units; KIND 0: sigma / S1, +inf for a primitive nothing reached.  In double, like flux_from_acc_kernel.
template <int KIND>
__global__ void flux_error_kernel(const unsigned long long *s1Acc, const unsigned long long *sqAcc, unsigned n, double numRays,
                                  float *out) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const double s1 = (double)s1Acc[i] * 9.094947017729282379150390625e-13; // 2^-40
  const double sq = (double)sqAcc[i] * 9.094947017729282379150390625e-13;
  const double sigma = sqrt(fmax(sq - s1 * s1 / numRays, 0.0));
  if (KIND == 1)
    out[i] = (float)sigma;
  else
    out[i] = s1Acc[i] == 0ull ? __int_as_float(0x7F800000) : (float)(sigma / s1);
}

hipError_t launch_stats_fill_absorbing(const unsigned long long *flux, unsigned n, unsigned long long *sumsq,
                                       unsigned long long *hits, hipStream_t st) {
  if (n == 0)
    return hipSuccess;
  hipLaunchKernelGGL(stats_fill_absorbing_kernel, dim3((n + 255) / 256), dim3(256), 0, st, flux, n, sumsq, hits);
  return hipGetLastError();
}

hipError_t launch_flux_error(const unsigned long long *s1, const unsigned long long *sumsq, unsigned n, double numRays,
                             int kind, float *out, hipStream_t st) {
  if (n == 0)
    return hipSuccess;
  if (kind == 1)
    hipLaunchKernelGGL(flux_error_kernel<1>, dim3((n + 255) / 256), dim3(256), 0, st, s1, sumsq, n, numRays, out);
  else
    hipLaunchKernelGGL(flux_error_kernel<0>, dim3((n + 255) / 256), dim3(256), 0, st, s1, sumsq, n, numRays, out);
  return hipGetLastError();
}

// un-permute the leaf-ordered accumulators into the caller's primitive order.
// Overflow is DETECTED, never silent: the accumulators are 64-bit fixed point (2^-40 per unit), summed over the replicas
// here and — as SIGNED int64 — over the ranks of a multi-GPU apply afterwards.  A primitive's sum must therefore stay
// below 2^(63 - headroomBits) (headroomBits = ceil(log2(ranks))): a replica with its top bit set, a carry out of the
// replica sum or a sum at or beyond that bound raises *overflowFlag, and vr_apply_finish fails the apply.
__global__ void gather_flux_kernel(const unsigned long long *acc, unsigned stride, unsigned replicas,
                                   const unsigned *leafOfOrig, unsigned n, unsigned long long *outAcc, unsigned headroomBits,
                                   unsigned long long *overflowFlag) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const unsigned q = leafOfOrig[i];
    unsigned long long s = 0; // (integer sum: replica order is irrelevant)
    bool bad = false;
    for (unsigned r = 0; r < replicas; ++r) {
      const unsigned long long v = acc[(size_t)r * stride + q];
      bad = bad || (v >> 63) != 0ull;
      s += v;
      bad = bad || s < v; // carry out of 64 bits
    }
    bad = bad || (s >> (63u - headroomBits)) != 0ull;
    outAcc[i] = s;
    if (bad)
      *overflowFlag = 1ull;
  }
}

hipError_t launch_gather_flux(const unsigned long long *acc, unsigned stride, unsigned replicas,
                              const unsigned *leafOfOrig, unsigned n, unsigned long long *outAcc, unsigned headroomBits,
                              unsigned long long *overflowFlag, hipStream_t s) {
  hipLaunchKernelGGL(gather_flux_kernel, dim3((n + 255) / 256), dim3(256), 0, s, acc, stride, replicas, leafOfOrig, n,
                     outAcc, headroomBits, overflowFlag);
  return hipGetLastError();
}

hipError_t launch_normalize_flux(float *flux, const float *area, unsigned n, int geo, int normType, float normFactor,
                                 double totalDiskArea, unsigned *maxOrd, hipStream_t st) {
  if (n == 0)
    return hipSuccess;
  const dim3 g((n + 255) / 256), b(256);
  if (normType == 0) {
    hipLaunchKernelGGL((normalize_flux_kernel<0, 0>), g, b, 0, st, flux, area, n, normFactor, totalDiskArea, maxOrd);
  } else {
    hipError_t e = hipMemsetAsync(maxOrd, 0, 4, st); // ordered 0 = below every float
    if (e != hipSuccess)
      return e;
    hipLaunchKernelGGL(flux_max_kernel, g, b, 0, st, flux, n, maxOrd);
    if (geo == 0)
      hipLaunchKernelGGL((normalize_flux_kernel<1, 0>), g, b, 0, st, flux, area, n, normFactor, totalDiskArea, maxOrd);
    else
      hipLaunchKernelGGL((normalize_flux_kernel<1, 1>), g, b, 0, st, flux, area, n, normFactor, totalDiskArea, maxOrd);
  }
  return hipGetLastError();
}

} // namespace vr
