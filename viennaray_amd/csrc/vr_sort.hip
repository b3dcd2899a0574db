// vr_sort.hip — the device primitives of the scene set-up: the in-place exclusive scan (radix-sort digit tables,
// neighbour offsets) and the LSD radix sort of (64-bit key, 32-bit value) pairs that orders the Morton codes.
#include <hip/hip_runtime.h>

#include "vr_kernels.hpp"
#include "vr_setup_common.hpp"
#include "vr_types.hpp"

namespace vr {

// ---------------------------------------------------------------------------
// exclusive scan (in place), 2048 elements per block: radix-sort digit tables, neighbour offsets
// ---------------------------------------------------------------------------
constexpr unsigned SCAN_PER_THREAD = 8;
constexpr unsigned SCAN_PER_BLOCK = SCAN_PER_THREAD * VR_BLOCK;

__device__ __forceinline__ unsigned block_exclusive_scan(unsigned v, unsigned *sh, unsigned &total) {
  const unsigned tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
  unsigned x = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    unsigned y = __shfl_up(x, off, 64);
    if ((int)lane >= off)
      x += y;
  }
  if (lane == 63)
    sh[w] = x;
  __syncthreads();
  unsigned base = 0;
  for (unsigned k = 0; k < w; ++k)
    base += sh[k];
  total = sh[0] + sh[1] + sh[2] + sh[3];
  __syncthreads();
  return base + x - v;
}

__global__ __launch_bounds__(VR_BLOCK) void scan_block_kernel(unsigned *data, unsigned n, unsigned *blockSums) {
  __shared__ unsigned sh[4];
  const unsigned base = blockIdx.x * SCAN_PER_BLOCK + threadIdx.x * SCAN_PER_THREAD;
  unsigned v[SCAN_PER_THREAD];
  unsigned sum = 0;
#pragma unroll
  for (unsigned k = 0; k < SCAN_PER_THREAD; ++k) {
    v[k] = base + k < n ? data[base + k] : 0u;
    sum += v[k];
  }
  unsigned total;
  unsigned ex = block_exclusive_scan(sum, sh, total);
#pragma unroll
  for (unsigned k = 0; k < SCAN_PER_THREAD; ++k) {
    if (base + k < n)
      data[base + k] = ex;
    ex += v[k];
  }
  if (threadIdx.x == 0 && blockSums)
    blockSums[blockIdx.x] = total;
}

__global__ __launch_bounds__(VR_BLOCK) void scan_add_kernel(unsigned *data, unsigned n, const unsigned *blockOffsets) {
  const unsigned off = blockOffsets[blockIdx.x];
  const unsigned base = blockIdx.x * SCAN_PER_BLOCK + threadIdx.x * SCAN_PER_THREAD;
#pragma unroll
  for (unsigned k = 0; k < SCAN_PER_THREAD; ++k)
    if (base + k < n)
      data[base + k] += off;
}

hipError_t launch_scan(unsigned *data, unsigned n, unsigned *tmp /* >= 2 * ceil(n/2048) + 2 */, hipStream_t s) {
  const unsigned blocks = (n + SCAN_PER_BLOCK - 1) / SCAN_PER_BLOCK;
  if (blocks <= 1) {
    hipLaunchKernelGGL(scan_block_kernel, dim3(1), dim3(VR_BLOCK), 0, s, data, n, (unsigned *)nullptr);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(scan_block_kernel, dim3(blocks), dim3(VR_BLOCK), 0, s, data, n, tmp);
  hipError_t e = launch_scan(tmp, blocks, tmp + blocks, s);
  if (e != hipSuccess)
    return e;
  hipLaunchKernelGGL(scan_add_kernel, dim3(blocks), dim3(VR_BLOCK), 0, s, data, n, tmp);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// LSD radix sort, one wavefront per tile of 1024 keys
// ---------------------------------------------------------------------------
constexpr unsigned SORT_TILE = 1024;

__global__ __launch_bounds__(64) void sort_count_kernel(const u64 *keys, unsigned n, unsigned shift, unsigned tiles,
                                                        unsigned *table) {
  __shared__ unsigned hist[256];
  const unsigned lane = threadIdx.x, tile = blockIdx.x;
  for (unsigned k = lane; k < 256; k += 64)
    hist[k] = 0;
  __syncthreads();
  for (unsigned it = 0; it < SORT_TILE / 64; ++it) {
    const unsigned idx = tile * SORT_TILE + it * 64 + lane;
    if (idx < n)
      atomicAdd(&hist[(unsigned)(keys[idx] >> shift) & 255u], 1u);
  }
  __syncthreads();
  for (unsigned k = lane; k < 256; k += 64)
    table[k * tiles + tile] = hist[k];
}

__global__ __launch_bounds__(64) void sort_scatter_kernel(const u64 *keysIn, const unsigned *valsIn, u64 *keysOut,
                                                          unsigned *valsOut, unsigned n, unsigned shift,
                                                          unsigned tiles, const unsigned *table) {
  __shared__ unsigned offs[256];
  const unsigned lane = threadIdx.x, tile = blockIdx.x;
  for (unsigned k = lane; k < 256; k += 64)
    offs[k] = table[k * tiles + tile];
  __syncthreads();
  const u64 ltMask = (1ull << lane) - 1ull;
  for (unsigned it = 0; it < SORT_TILE / 64; ++it) {
    const unsigned idx = tile * SORT_TILE + it * 64 + lane;
    const bool valid = idx < n;
    u64 key = 0;
    unsigned val = 0, d = 0;
    if (valid) {
      key = keysIn[idx];
      val = valsIn[idx];
      d = (unsigned)(key >> shift) & 255u;
    }
    // lanes holding the same digit: AND of 8 per-bit ballots
    u64 peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const u64 m = __ballot(valid && ((d >> b) & 1u));
      peers &= ((d >> b) & 1u) ? m : ~m;
    }
    if (valid) {
      const unsigned rank = __popcll(peers & ltMask);
      const unsigned base = offs[d];
      keysOut[base + rank] = key;
      valsOut[base + rank] = val;
      if (rank == 0)
        offs[d] = base + __popcll(peers); // in-order LDS: every peer has read `base`
    }
  }
}

// (keysA, valsA) -> ping-pong with (keysB, valsB), 8 passes end in A (vr_kernels.hpp has the buffer sizes)
hipError_t launch_sort_pairs(u64 *keysA, unsigned *valsA, u64 *keysB, unsigned *valsB, unsigned n, unsigned *sortTable,
                             unsigned *scanTmp, hipStream_t st) {
  hipError_t e = hipSuccess;
  const unsigned tiles = (n + SORT_TILE - 1) / SORT_TILE;
  u64 *kin = keysA, *kout = keysB;
  unsigned *vin = valsA, *vout = valsB;
  for (unsigned pass = 0; pass < 8; ++pass) {
    hipLaunchKernelGGL(sort_count_kernel, dim3(tiles), dim3(64), 0, st, kin, n, pass * 8, tiles, sortTable);
    e = launch_scan(sortTable, 256u * tiles, scanTmp, st);
    if (e != hipSuccess)
      return e;
    hipLaunchKernelGGL(sort_scatter_kernel, dim3(tiles), dim3(64), 0, st, kin, vin, kout, vout, n, pass * 8, tiles,
                       sortTable);
    u64 *tk = kin;
    kin = kout;
    kout = tk;
    unsigned *tv = vin;
    vin = vout;
    vout = tv;
  }
  // (8 passes: result is back in A)
  return e;
}

} // namespace vr
