// vr_ingest.hip — device-resident inputs: what the host setters make of the caller's arrays, made from rows that are
// already in HBM — the discs' records, the disk and mesh ingest with their bounding boxes, the sort-plane histogram, the
// global-data rows, the per-primitive sticking and the surface-source tables.
#include <hip/hip_runtime.h>

#include "vr_kernels.hpp"
#include "vr_setup_common.hpp"
#include "vr_types.hpp"

namespace vr {

// the discs' {centre, radius} records from the caller's points (one radius for all: rayGeometryDisk.hpp:60-75; 2-D: the z
// column is ignored) — 16 bytes per disk that need not cross PCIe
__global__ void disk4_kernel(const float *points3, unsigned n, float radius, int D, float4 *disk4) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n)
    disk4[i] = make_float4(points3[3 * (size_t)i], points3[3 * (size_t)i + 1], D == 2 ? 0.f : points3[3 * (size_t)i + 2], radius);
}
hipError_t launch_disk4(const float *points3, unsigned n, float radius, int D, float *disk4, hipStream_t st) {
  if (n)
    hipLaunchKernelGGL(disk4_kernel, dim3((n + 255) / 256), dim3(256), 0, st, points3, n, radius, D, reinterpret_cast<float4 *>(disk4));
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Device-resident disk geometry (vr_set_disks_device): the caller's rows are already in HBM, so what host_set_disks
// and host_sort_plane do in host threads is done here — the packed copies the builder reads, the bounding box and the
// sort-plane histogram.  What comes back to the host: six floats at set time, 512 doubles at prepare time.
// ---------------------------------------------------------------------------
// Key of a coordinate for the box reductions.  The host loop (host_set_disks) keeps the FIRST row among equal values
// (std::min / std::max replace on a strict compare, threads merged in index order), and -0 == +0: which zero it ends with
// depends on the row order.  So the high word orders by value with both zeros folded into one, and the low word makes
// the lowest row index win among equals and carries that row's sign bit (rows < 2^27).  NaNs never win a compare on the
// host: they map to the identity here.
constexpr u64 kMinIdentity = ((u64)0xFF7FFFFFu << 32) | 0xFFFFFFFFull; // f2ord(FLT_MAX), behind every row
constexpr u64 kMaxIdentity = ((u64)0x00800000u << 32);                 // f2ord(-FLT_MAX), behind every row
__device__ __forceinline__ u64 box_min_key(float v, unsigned row) {
  if (!(v == v))
    return kMinIdentity;
  const u64 sign = __float_as_uint(v) >> 31;
  return ((u64)f2ord(v == 0.f ? 0.f : v) << 32) | ((u64)row << 1) | sign;
}
__device__ __forceinline__ u64 box_max_key(float v, unsigned row) {
  if (!(v == v))
    return kMaxIdentity;
  const u64 sign = __float_as_uint(v) >> 31;
  return ((u64)f2ord(v == 0.f ? 0.f : v) << 32) | ((u64)(0x7FFFFFFFu - row) << 1) | sign;
}
__device__ __forceinline__ float box_key_value(u64 key) {
  const float v = ord2f((unsigned)(key >> 32));
  return (v == 0.f && (key & 1ull)) ? -0.f : v;
}
__device__ __forceinline__ u64 wave_min_u64(u64 v) {
  for (int off = 32; off > 0; off >>= 1) {
    const u64 o = __shfl_down(v, off, 64);
    v = o < v ? o : v;
  }
  return v;
}
__device__ __forceinline__ u64 wave_max_u64(u64 v) {
  for (int off = 32; off > 0; off >>= 1) {
    const u64 o = __shfl_down(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}

constexpr unsigned INGEST_ROWS = 256;        // rows per tile = threads per block
constexpr unsigned INGEST_MAX_BLOCKS = 1024; // grid-stride over the tiles; one set of six partial keys per block

// One pass over the caller's rows (ld = 2 or 3 floats each; ld == 2 only with D == 2).  A tile of 256 rows is read as
// the flat run of floats it is (consecutive lanes, consecutive addresses, whatever ld), staged in LDS, and written the
// same way as packed rows of 3 with the z column zeroed for D == 2: points3 / normal3 are what host_set_disks makes,
// disk4 what disk4_kernel makes of points3.  The box of the first D columns is reduced per wave, per block, and left as
// six keys per block for ingest_bounds_kernel.
__global__ __launch_bounds__(256) void ingest_disks_kernel(const float *pts, const float *nrm, unsigned n, unsigned ld,
                                                           int D, float radius, float *points3, float *normal3,
                                                           float4 *disk4, u64 *partials) {
  __shared__ float sp[INGEST_ROWS * 3], sn[INGEST_ROWS * 3];
  __shared__ u64 red[4][6];
  u64 kmin[3] = {kMinIdentity, kMinIdentity, kMinIdentity}, kmax[3] = {kMaxIdentity, kMaxIdentity, kMaxIdentity};
  const unsigned tiles = (n + INGEST_ROWS - 1) / INGEST_ROWS;
  for (unsigned t = blockIdx.x; t < tiles; t += gridDim.x) {
    const unsigned row0 = t * INGEST_ROWS, rows = min(INGEST_ROWS, n - row0);
    const size_t in0 = (size_t)row0 * ld, out0 = (size_t)row0 * 3;
    for (unsigned j = threadIdx.x; j < rows * ld; j += INGEST_ROWS) {
      sp[j] = pts[in0 + j];
      sn[j] = nrm[in0 + j];
    }
    __syncthreads();
    for (unsigned j = threadIdx.x; j < rows * 3; j += INGEST_ROWS) {
      const unsigned r = j / 3, col = j - 3 * r;
      const bool zero = col == 2 && D == 2; // (covers ld == 2: it comes with D == 2 only)
      points3[out0 + j] = zero ? 0.f : sp[r * ld + col];
      normal3[out0 + j] = zero ? 0.f : sn[r * ld + col];
    }
    if (threadIdx.x < rows) {
      const unsigned r = threadIdx.x, row = row0 + r;
      const float x = sp[r * ld], y = sp[r * ld + 1], z = D == 2 ? 0.f : sp[r * ld + 2];
      disk4[row] = make_float4(x, y, z, radius);
      const float p[3] = {x, y, z};
      for (int k = 0; k < D; ++k) {
        const u64 a = box_min_key(p[k], row), b = box_max_key(p[k], row);
        kmin[k] = a < kmin[k] ? a : kmin[k];
        kmax[k] = b > kmax[k] ? b : kmax[k];
      }
    }
    __syncthreads(); // (the next tile overwrites the staging)
  }
  for (int k = 0; k < 3; ++k) {
    const u64 a = wave_min_u64(kmin[k]), b = wave_max_u64(kmax[k]);
    if ((threadIdx.x & 63) == 0) {
      red[threadIdx.x >> 6][k] = a;
      red[threadIdx.x >> 6][3 + k] = b;
    }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    u64 v = red[0][threadIdx.x];
    for (int w = 1; w < 4; ++w) {
      const u64 o = red[w][threadIdx.x];
      v = threadIdx.x < 3 ? (o < v ? o : v) : (o > v ? o : v);
    }
    partials[6 * (size_t)blockIdx.x + threadIdx.x] = v;
  }
}

// block k (one wave) merges key k of every block of ingest_disks_kernel: bounds6 = {min xyz, max xyz} as floats
__global__ __launch_bounds__(64) void ingest_bounds_kernel(const u64 *partials, unsigned blocks, float *bounds6) {
  const unsigned k = blockIdx.x;
  u64 v = k < 3 ? kMinIdentity : kMaxIdentity;
  for (unsigned b = threadIdx.x; b < blocks; b += 64) {
    const u64 o = partials[6 * (size_t)b + k];
    v = k < 3 ? (o < v ? o : v) : (o > v ? o : v);
  }
  v = k < 3 ? wave_min_u64(v) : wave_max_u64(v);
  if (threadIdx.x == 0)
    bounds6[k] = box_key_value(v);
}

size_t ingest_partials_entries() { return 6 * (size_t)INGEST_MAX_BLOCKS; }

hipError_t launch_ingest_disks(const float *pts, const float *nrm, unsigned n, unsigned ld, int D, float radius,
                               float *points3, float *normal3, float *disk4, unsigned long long *partials, float *bounds6,
                               hipStream_t st) {
  const unsigned tiles = (n + INGEST_ROWS - 1) / INGEST_ROWS;
  const unsigned blocks = tiles < INGEST_MAX_BLOCKS ? tiles : INGEST_MAX_BLOCKS;
  if (blocks)
    hipLaunchKernelGGL(ingest_disks_kernel, dim3(blocks), dim3(INGEST_ROWS), 0, st, pts, nrm, n, ld, D, radius, points3,
                       normal3, reinterpret_cast<float4 *>(disk4), partials);
  hipLaunchKernelGGL(ingest_bounds_kernel, dim3(6), dim3(64), 0, st, partials, blocks, bounds6); // (no rows: the identities)
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Device-resident triangle mesh (vr_set_triangles_device), in two passes.  The first only reads the caller's buffers:
// nothing resident may change before every index is known to be good.  The second, launched once the host has seen the
// first one's seven words, makes what host_set_triangles makes.
// ---------------------------------------------------------------------------
constexpr unsigned kNoBadTriangle = 0xFFFFFFFFu;

// Pass 1.  Both buffers are read as the flat runs they are (consecutive lanes, consecutive addresses).  The box of ALL
// vertices, all three columns whatever D is (rayMesh.hpp:12-25), is reduced as ingest_disks_kernel reduces it and left
// as six keys per block for ingest_bounds_kernel.  An index >= nverts is only compared, never followed: the lowest
// triangle that holds one is reduced per wave, per block, and one atomic min per block (its result unused) leaves it in
// *badTri (kNoBadTriangle before the launch).
__global__ __launch_bounds__(256) void scan_mesh_kernel(const float *verts, unsigned nverts, const unsigned *tris,
                                                        unsigned ntris, u64 *partials, unsigned *badTri) {
  __shared__ u64 red[4][6];
  __shared__ unsigned redBad[4];
  u64 kmin[3] = {kMinIdentity, kMinIdentity, kMinIdentity}, kmax[3] = {kMaxIdentity, kMaxIdentity, kMaxIdentity};
  const size_t step = (size_t)gridDim.x * INGEST_ROWS;
  const size_t nf = (size_t)nverts * 3;
  for (size_t j = (size_t)blockIdx.x * INGEST_ROWS + threadIdx.x; j < nf; j += step) {
    const unsigned row = (unsigned)(j / 3), col = (unsigned)(j - 3 * (size_t)row);
    const float v = verts[j];
    const u64 a = box_min_key(v, row), b = box_max_key(v, row);
#pragma unroll
    for (unsigned k = 0; k < 3; ++k) { // (static register indices: the column only selects)
      kmin[k] = (col == k && a < kmin[k]) ? a : kmin[k];
      kmax[k] = (col == k && b > kmax[k]) ? b : kmax[k];
    }
  }
  unsigned bad = kNoBadTriangle;
  const size_t ni = (size_t)ntris * 3;
  for (size_t j = (size_t)blockIdx.x * INGEST_ROWS + threadIdx.x; j < ni; j += step)
    if (tris[j] >= nverts) {
      const unsigned t = (unsigned)(j / 3);
      bad = t < bad ? t : bad;
    }
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned o = __shfl_down(bad, off, 64);
    bad = o < bad ? o : bad;
  }
  for (int k = 0; k < 3; ++k) {
    const u64 a = wave_min_u64(kmin[k]), b = wave_max_u64(kmax[k]);
    if ((threadIdx.x & 63) == 0) {
      red[threadIdx.x >> 6][k] = a;
      red[threadIdx.x >> 6][3 + k] = b;
    }
  }
  if ((threadIdx.x & 63) == 0)
    redBad[threadIdx.x >> 6] = bad;
  __syncthreads();
  if (threadIdx.x < 6) {
    u64 v = red[0][threadIdx.x];
    for (int w = 1; w < 4; ++w) {
      const u64 o = red[w][threadIdx.x];
      v = threadIdx.x < 3 ? (o < v ? o : v) : (o > v ? o : v);
    }
    partials[6 * (size_t)blockIdx.x + threadIdx.x] = v;
  }
  if (threadIdx.x == 64) { // (another wave than the one that writes the keys)
    const unsigned b = min(min(redBad[0], redBad[1]), min(redBad[2], redBad[3]));
    if (b != kNoBadTriangle)
      atomicMin(badTri, b);
  }
}

hipError_t launch_scan_mesh(const float *verts, unsigned nverts, const unsigned *tris, unsigned ntris,
                            unsigned long long *partials, float *bounds6, unsigned *badTri, hipStream_t st) {
  hipError_t e = hipMemsetAsync(badTri, 0xFF, sizeof(unsigned), st);
  if (e != hipSuccess)
    return e;
  const size_t rows = nverts > ntris ? nverts : ntris;
  const size_t tiles = (rows * 3 + INGEST_ROWS - 1) / INGEST_ROWS;
  const unsigned blocks = (unsigned)(tiles < INGEST_MAX_BLOCKS ? tiles : INGEST_MAX_BLOCKS);
  if (blocks)
    hipLaunchKernelGGL(scan_mesh_kernel, dim3(blocks), dim3(INGEST_ROWS), 0, st, verts, nverts, tris, ntris, partials,
                       badTri);
  hipLaunchKernelGGL(ingest_bounds_kernel, dim3(6), dim3(64), 0, st, partials, blocks, bounds6);
  return hipGetLastError();
}

// Pass 2 (every index < nverts).  The vertices are copied as a flat run.  A tile of 256 triangles: its 768 indices are
// read flat into LDS and written flat to outTris; thread r then gathers the three vertices of triangle r and computes the
// normal and the area with host_set_triangles' operations in its order (vr_host.cpp: cross3 of v1 - v0 and v2 - v0, the
// dot product summed (x + y) + z, sqrtf, three divisions, a zero-length normal left as it is; area = (float)(0.5 * norm)
// with the product in double; D == 2: the even / odd edge rule of rayGeometryTriangle.hpp:62-75).  The normals leave
// through LDS, flat again.
__global__ __launch_bounds__(256) void pack_mesh_kernel(const float *verts, unsigned nverts, const unsigned *tris,
                                                        unsigned ntris, int D, float *outVerts, unsigned *outTris,
                                                        float *normal3, float *areas) {
  __shared__ unsigned si[INGEST_ROWS * 3];
  __shared__ float sn[INGEST_ROWS * 3];
  const size_t step = (size_t)gridDim.x * INGEST_ROWS;
  const size_t nf = (size_t)nverts * 3;
  for (size_t j = (size_t)blockIdx.x * INGEST_ROWS + threadIdx.x; j < nf; j += step)
    outVerts[j] = verts[j];
  const unsigned tiles = (ntris + INGEST_ROWS - 1) / INGEST_ROWS;
  for (unsigned t = blockIdx.x; t < tiles; t += gridDim.x) {
    const unsigned row0 = t * INGEST_ROWS, rows = min(INGEST_ROWS, ntris - row0);
    const size_t o0 = (size_t)row0 * 3;
    for (unsigned j = threadIdx.x; j < rows * 3; j += INGEST_ROWS) {
      const unsigned v = tris[o0 + j];
      si[j] = v;
      outTris[o0 + j] = v;
    }
    __syncthreads();
    if (threadIdx.x < rows) {
      const unsigned r = threadIdx.x, i = row0 + r;
      const float *a = verts + 3 * (size_t)si[3 * r], *b = verts + 3 * (size_t)si[3 * r + 1],
                  *c = verts + 3 * (size_t)si[3 * r + 2];
      // (plain operators: the build has -ffp-contract=off, and sqrt and division are the IEEE ones, as in vr_area.hpp)
      const float ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2]; // v1 - v0
      const float wx = c[0] - a[0], wy = c[1] - a[1], wz = c[2] - a[2]; // v2 - v0
      float nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
      const float nn = __builtin_sqrtf((nx * nx + ny * ny) + nz * nz);
      float len = nn; // (what the area is half of)
      if (D == 2) {
        const float ex = (i & 1u) ? wx : ux, ey = (i & 1u) ? wy : uy, ez = (i & 1u) ? wz : uz;
        len = __builtin_sqrtf((ex * ex + ey * ey) + ez * ez);
      }
      areas[i] = (float)(0.5 * (double)len);
      if (!(nn <= 0.f)) { // (normalize3 returns on n <= 0; a NaN length divides, as there)
        nx /= nn;
        ny /= nn;
        nz /= nn;
      }
      sn[3 * r] = nx;
      sn[3 * r + 1] = ny;
      sn[3 * r + 2] = nz;
    }
    __syncthreads();
    for (unsigned j = threadIdx.x; j < rows * 3; j += INGEST_ROWS)
      normal3[o0 + j] = sn[j];
    // (no barrier here: the next tile writes si, last read before the barrier above, and writes sn only behind its own
    //  first barrier, which every thread reaches after these reads)
  }
}

hipError_t launch_pack_mesh(const float *verts, unsigned nverts, const unsigned *tris, unsigned ntris, int D,
                            float *outVerts, unsigned *outTris, float *normal3, float *areas, hipStream_t st) {
  const size_t rows = nverts > ntris ? nverts : ntris;
  const size_t tiles = (rows + INGEST_ROWS - 1) / INGEST_ROWS;
  const unsigned blocks = (unsigned)(tiles < INGEST_MAX_BLOCKS ? tiles : INGEST_MAX_BLOCKS);
  if (!blocks)
    return hipSuccess;
  hipLaunchKernelGGL(pack_mesh_kernel, dim3(blocks), dim3(INGEST_ROWS), 0, st, verts, nverts, tris, ntris, D, outVerts,
                     outTris, normal3, areas);
  return hipGetLastError();
}

// host_sort_plane on the device: 256 slices of [lo, hi] on the sort axis, each primitive adds the area it shows the source
// and that area times its coordinate, in double — a disk (GEO 0) r^2 |n_axis| / |n| at its centre, a triangle (GEO 1)
// the area of its projection along the axis at its centroid (vr_host.cpp, the two branches of host_sort_plane's loop).
// Double sums depend on their order, so the order is
// fixed: a block takes one contiguous range of primitives, a wave its 64-primitive runs in turn; within a run the lanes of
// one slice are summed by a butterfly (the same tree on every run) and added once to the wave's own LDS histogram; the
// waves, then the blocks (sort_plane_merge_kernel), are merged in index order.  The same input gives the same bits.
constexpr int SORT_SLICES = 256;
constexpr unsigned SORT_MAX_BLOCKS = 256;
// GEO 0: disk4 / normal3;  GEO 1: verts / tris (passed in their places)
template <int GEO>
__global__ __launch_bounds__(256) void sort_plane_kernel(const float4 *disk4, const float *normal3, const float *verts,
                                                         const unsigned *tris, unsigned n, int axis, float lo, float hi,
                                                         double *partials) {
  __shared__ double hw[4][SORT_SLICES], hwh[4][SORT_SLICES];
  for (unsigned j = threadIdx.x; j < 4 * SORT_SLICES; j += 256) {
    (&hw[0][0])[j] = 0.;
    (&hwh[0][0])[j] = 0.;
  }
  __syncthreads();
  const double inv = SORT_SLICES / ((double)hi - (double)lo);
  const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const unsigned perBlock = (((n + gridDim.x - 1) / gridDim.x) + 255u) & ~255u;
  const unsigned begin = min(n, blockIdx.x * perBlock), end = min(n, begin + perBlock);
  for (unsigned base = begin + wave * 64; base < end; base += 256) { // (wave-uniform)
    const unsigned i = base + lane;
    const bool valid = i < end;
    int k = -1;
    double a = 0., ah = 0.;
    if (valid) {
      double h;
      if constexpr (GEO == 0) {
        const float4 d = disk4[i];
        const float nx = normal3[3 * (size_t)i], ny = normal3[3 * (size_t)i + 1], nz = normal3[3 * (size_t)i + 2];
        const double nn = sqrt((double)nx * nx + (double)ny * ny + (double)nz * nz);
        h = axis == 0 ? d.x : axis == 1 ? d.y : d.z;
        const float na = axis == 0 ? nx : axis == 1 ? ny : nz;
        a = nn > 0. ? (double)d.w * d.w * fabs((double)na) / nn : 0.;
      } else {
        const float *v0 = verts + 3 * (size_t)tris[3 * (size_t)i], *v1 = verts + 3 * (size_t)tris[3 * (size_t)i + 1],
                    *v2 = verts + 3 * (size_t)tris[3 * (size_t)i + 2];
        const int a1 = (axis + 1) % 3, a2 = (axis + 2) % 3;
        const double e10 = (double)v1[a1] - v0[a1], e11 = (double)v1[a2] - v0[a2];
        const double e20 = (double)v2[a1] - v0[a1], e21 = (double)v2[a2] - v0[a2];
        h = ((double)v0[axis] + v1[axis] + v2[axis]) / 3.;
        a = 0.5 * fabs(e10 * e21 - e11 * e20);
      }
      ah = a * h;
      k = (int)((h - lo) * inv);
      k = k < 0 ? 0 : (k >= SORT_SLICES ? SORT_SLICES - 1 : k);
    }
    u64 todo = __ballot(valid);
    while (todo) { // one slice per turn, lowest waiting lane first
      const int kk = __shfl(k, __ffsll((long long)todo) - 1, 64);
      const bool mine = valid && k == kk;
      double sa = mine ? a : 0., sah = mine ? ah : 0.;
      for (int off = 32; off > 0; off >>= 1) {
        sa += __shfl_xor(sa, off, 64);
        sah += __shfl_xor(sah, off, 64);
      }
      if (lane == 0) {
        hw[wave][kk] += sa;
        hwh[wave][kk] += sah;
      }
      todo &= ~__ballot(mine);
    }
  }
  __syncthreads();
  const unsigned j = threadIdx.x; // (256 threads = SORT_SLICES)
  partials[(2 * (size_t)blockIdx.x) * SORT_SLICES + j] = ((hw[0][j] + hw[1][j]) + hw[2][j]) + hw[3][j];
  partials[(2 * (size_t)blockIdx.x + 1) * SORT_SLICES + j] = ((hwh[0][j] + hwh[1][j]) + hwh[2][j]) + hwh[3][j];
}

// hist[0 .. 255] = area per slice, hist[256 .. 511] = area x coordinate per slice: the blocks' partials in block order
__global__ __launch_bounds__(256) void sort_plane_merge_kernel(const double *partials, unsigned blocks, double *hist) {
  const unsigned j = blockIdx.x * 256 + threadIdx.x; // < 2 * SORT_SLICES
  double s = 0.;
  for (unsigned b = 0; b < blocks; ++b)
    s += partials[(2 * (size_t)b) * SORT_SLICES + j];
  hist[j] = s;
}

size_t sort_plane_partials_entries() { return 2 * (size_t)SORT_SLICES * SORT_MAX_BLOCKS; }

hipError_t launch_sort_plane(int geo, const float *disk4, const float *normal3, const float *verts, const unsigned *tris,
                             unsigned n, int axis, float lo, float hi, double *partials, double *hist512, hipStream_t st) {
  if (n == 0)
    return hipSuccess;
  const unsigned tiles = (n + 255) / 256;
  const unsigned blocks = tiles < SORT_MAX_BLOCKS ? tiles : SORT_MAX_BLOCKS;
  if (geo == 0)
    hipLaunchKernelGGL(sort_plane_kernel<0>, dim3(blocks), dim3(256), 0, st, reinterpret_cast<const float4 *>(disk4),
                       normal3, verts, tris, n, axis, lo, hi, partials);
  else
    hipLaunchKernelGGL(sort_plane_kernel<1>, dim3(blocks), dim3(256), 0, st, reinterpret_cast<const float4 *>(disk4),
                       normal3, verts, tris, n, axis, lo, hi, partials);
  hipLaunchKernelGGL(sort_plane_merge_kernel, dim3(2), dim3(256), 0, st, partials, blocks, hist512);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Device-resident inputs of a time step (vr_set_global_data_device, vr_set_material_ids_device,
// vr_set_surface_source_device): streaming kernels, one thread per element or row, grid-stride.
// ---------------------------------------------------------------------------
constexpr unsigned INPUT_MAX_BLOCKS = 2048;
static unsigned input_blocks(size_t n) {
  const size_t b = (n + 255) / 256;
  return (unsigned)(b < INPUT_MAX_BLOCKS ? (b ? b : 1) : INPUT_MAX_BLOCKS);
}

// one row of the global data: dst[0 .. stride) = src[0 .. n), zeros behind it
__global__ __launch_bounds__(256) void global_row_kernel(const float *src, unsigned n, float *dst, unsigned stride) {
  for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < stride; i += gridDim.x * 256)
    dst[i] = i < n ? src[i] : 0.f;
}
hipError_t launch_global_row(const float *src, unsigned n, float *dst, unsigned stride, hipStream_t st) {
  if (stride == 0)
    return hipSuccess;
  hipLaunchKernelGGL(global_row_kernel, dim3(input_blocks(stride)), dim3(256), 0, st, src, n, dst, stride);
  return hipGetLastError();
}

// the global data re-laid at another stride / row count: dst[newRows][newStride] = src[oldRows][oldStride], zeros elsewhere
__global__ __launch_bounds__(256) void global_relayout_kernel(const float *src, unsigned oldRows, unsigned oldStride,
                                                              float *dst, unsigned newRows, unsigned newStride) {
  const size_t total = (size_t)newRows * newStride;
  for (size_t j = (size_t)blockIdx.x * 256 + threadIdx.x; j < total; j += (size_t)gridDim.x * 256) {
    const unsigned r = (unsigned)(j / newStride), i = (unsigned)(j - (size_t)r * newStride);
    dst[j] = (r < oldRows && i < oldStride) ? src[(size_t)r * oldStride + i] : 0.f;
  }
}
hipError_t launch_global_relayout(const float *src, unsigned oldRows, unsigned oldStride, float *dst, unsigned newRows,
                                  unsigned newStride, hipStream_t st) {
  const size_t total = (size_t)newRows * newStride;
  if (total == 0)
    return hipSuccess;
  hipLaunchKernelGGL(global_relayout_kernel, dim3(input_blocks(total)), dim3(256), 0, st, src, oldRows, oldStride, dst,
                     newRows, newStride);
  return hipGetLastError();
}

// per-primitive sticking in leaf order from the material ids in the caller's order (prepare_sticking): the particle's
// (id, value) table is searched to its end, so the last entry of an id wins as in the reference's map; a primitive
// beyond the ids given has id 0
__global__ __launch_bounds__(256) void prim_sticking_kernel(const unsigned *order, const int *ids, unsigned numIds,
                                                            const int *tabIds, const float *tabVals, unsigned tabN,
                                                            float base, unsigned n, float *out) {
  for (unsigned q = blockIdx.x * 256 + threadIdx.x; q < n; q += gridDim.x * 256) {
    const unsigned o = order[q];
    const int mat = o < numIds ? ids[o] : 0;
    float s = base;
    for (unsigned m = 0; m < tabN; ++m)
      if (tabIds[m] == mat)
        s = tabVals[m];
    out[q] = s;
  }
}
hipError_t launch_prim_sticking(const unsigned *order, const int *ids, unsigned numIds, const int *tabIds,
                                const float *tabVals, unsigned tabN, float base, unsigned n, float *out, hipStream_t st) {
  if (n == 0)
    return hipSuccess;
  hipLaunchKernelGGL(prim_sticking_kernel, dim3(input_blocks(n)), dim3(256), 0, st, order, ids, numIds, tabIds, tabVals,
                     tabN, base, n, out);
  return hipGetLastError();
}

// The surface-source tables from device rows (ld = 2 or 3 floats; a missing third column reads 0): packed into
// pos3 / nrm3 / w and checked row by row as vr_set_surface_source checks them — position finite, normal length (the same
// sums in the same order) positive and finite, weight >= 0 and finite.  *bad ends as the smallest row * 4 + kind
// (0 position, 1 normal, 2 weight) of the failing checks, each row reporting its first: the host loop's first refusal.
__global__ __launch_bounds__(256) void surface_source_kernel(const float *pos, const float *nrm, const float *wgt,
                                                             unsigned n, unsigned ld, float *pos3, float *nrm3, float *w,
                                                             u64 *bad) {
  u64 worst = ~0ull;
  for (unsigned j = blockIdx.x * 256 + threadIdx.x; j < n; j += gridDim.x * 256) {
    const float *q = pos + (size_t)j * ld, *m = nrm + (size_t)j * ld;
    const float q0 = q[0], q1 = q[1], q2 = ld == 3 ? q[2] : 0.f;
    const float m0 = m[0], m1 = m[1], m2 = ld == 3 ? m[2] : 0.f;
    const float wj = wgt[j];
    pos3[3 * (size_t)j] = q0;
    pos3[3 * (size_t)j + 1] = q1;
    pos3[3 * (size_t)j + 2] = q2;
    nrm3[3 * (size_t)j] = m0;
    nrm3[3 * (size_t)j + 1] = m1;
    nrm3[3 * (size_t)j + 2] = m2;
    w[j] = wj;
    const float len = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(m0, m0), __fmul_rn(m1, m1)), __fmul_rn(m2, m2)));
    int kind = -1;
    if (!isfinite(q0) || !isfinite(q1) || !isfinite(q2))
      kind = 0;
    else if (!(len > 0.f) || !isfinite(len))
      kind = 1;
    else if (!(wj >= 0.f) || !isfinite(wj))
      kind = 2;
    if (kind >= 0) {
      const u64 key = (u64)j * 4u + (u64)kind;
      worst = key < worst ? key : worst;
    }
  }
  worst = wave_min_u64(worst); // (lane 0 holds the wave's smallest)
  if ((threadIdx.x & 63) == 0 && worst != ~0ull)
    atomicMin(bad, worst);
}
hipError_t launch_surface_source(const float *pos, const float *nrm, const float *wgt, unsigned n, unsigned ld,
                                 float *pos3, float *nrm3, float *w, unsigned long long *bad, hipStream_t st) {
  hipError_t e = hipMemsetAsync(bad, 0xFF, sizeof(u64), st);
  if (e != hipSuccess || n == 0)
    return e;
  hipLaunchKernelGGL(surface_source_kernel, dim3(input_blocks(n)), dim3(256), 0, st, pos, nrm, wgt, n, ld, pos3, nrm3, w,
                     bad);
  return hipGetLastError();
}

} // namespace vr
