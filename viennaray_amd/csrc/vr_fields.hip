// vr_fields.hip — the two fields over the source plane that every prepare builds from the resident primitive records:
// the height field (HeightFieldParams) and the relief field (ReliefParams), both in vr_types.hpp; and the one per-scene
// fact a geometry commit reads off those records: whether the disks are uniform (launch_uniform_disks); and the lattice
// table of a planar cloud (launch_lattice_table).
#include <hip/hip_runtime.h>

#include "vr_kernels.hpp"
#include "vr_planar_lattice.hpp"
#include "vr_setup_common.hpp"
#include "vr_types.hpp"

namespace vr {

// ---------------------------------------------------------------------------
// height field over the source plane (HeightFieldParams, vr_types.hpp)
// ---------------------------------------------------------------------------
__global__ void height_field_kernel(HeightFieldParams q) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= q.n)
    return;
  const float4 *pr = reinterpret_cast<const float4 *>(q.prims);
  float lo[3], hi[3];
  if (q.geo == 0) {
    const float4 c = pr[2 * (size_t)i], n = pr[2 * (size_t)i + 1];
    const float cc[3] = {c.x, c.y, c.z}, nn[3] = {n.x, n.y, n.z};
    for (int k = 0; k < 3; ++k) { // the disc's own extent along axis k (as the BVH's boxes: vr_bvh.hip, prim_box_kernel)
      const float e = c.w * sqrtf(fmaxf(0.f, 1.f - nn[k] * nn[k])) * 1.0001f;
      lo[k] = cc[k] - e;
      hi[k] = cc[k] + e;
    }
  } else {
    const float4 a = pr[4 * (size_t)i], e1 = pr[4 * (size_t)i + 1], e2 = pr[4 * (size_t)i + 2];
    const float v0[3] = {a.x, a.y, a.z}, v1[3] = {a.x - e1.x, a.y - e1.y, a.z - e1.z}, v2[3] = {a.x + e2.x, a.y + e2.y, a.z + e2.z};
    for (int k = 0; k < 3; ++k) {
      lo[k] = fminf(v0[k], fminf(v1[k], v2[k]));
      hi[k] = fmaxf(v0[k], fmaxf(v1[k], v2[k]));
    }
  }
  const float top = (q.sign > 0.f ? hi[q.ax] : -lo[q.ax]) + q.pad;
  const int ix0 = min(max((int)floorf((lo[q.a1] - q.pad - q.lo1) * q.invTile), 0), q.nx - 1);
  const int ix1 = min(max((int)floorf((hi[q.a1] + q.pad - q.lo1) * q.invTile), 0), q.nx - 1);
  int iy0 = 0, iy1 = 0;
  if (q.ny > 1) {
    iy0 = min(max((int)floorf((lo[q.a2] - q.pad - q.lo2) * q.invTile), 0), q.ny - 1);
    iy1 = min(max((int)floorf((hi[q.a2] + q.pad - q.lo2) * q.invTile), 0), q.ny - 1);
  }
  for (int iy = iy0; iy <= iy1; ++iy)
    for (int ix = ix0; ix <= ix1; ++ix)
      atomicMax(&q.raw[iy * q.nx + ix], f2ord(top));
}

__global__ void height_dilate_kernel(HeightFieldParams q) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= q.nx * q.ny)
    return;
  const int ix = t % q.nx, iy = t / q.nx;
  unsigned m = 0u; // (f2ord: 0 is below every float — a tile nothing reaches into)
  for (int dy = -1; dy <= 1; ++dy)
    for (int dx = -1; dx <= 1; ++dx) {
      const int x = ix + dx, y = iy + dy;
      if (x >= 0 && x < q.nx && y >= 0 && y < q.ny)
        m = max(m, q.raw[y * q.nx + x]);
    }
  q.field[t] = m ? ord2f(m) : -3.0e38f;
}

hipError_t launch_height_field(const HeightFieldParams &q, hipStream_t st) {
  hipError_t e = hipMemsetAsync(q.raw, 0, (size_t)q.nx * q.ny * 4, st);
  if (e != hipSuccess)
    return e;
  if (q.n)
    hipLaunchKernelGGL(height_field_kernel, dim3((q.n + 255) / 256), dim3(256), 0, st, q);
  hipLaunchKernelGGL(height_dilate_kernel, dim3((q.nx * q.ny + 255) / 256), dim3(256), 0, st, q);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// relief field over the source plane (ReliefParams, vr_types.hpp): fine tiles {lo, hi} for the tracer's per-ray clip
// (relief_clip), coarse tiles {mid height, largest fine thickness} for the generator's sort key
// ---------------------------------------------------------------------------
__device__ __forceinline__ void relief_prim_box(const ReliefParams &q, unsigned i, float (&lo)[3], float (&hi)[3]) {
  const float4 *pr = reinterpret_cast<const float4 *>(q.prims);
  if (q.geo == 0) {
    const float4 c = pr[2 * (size_t)i], n = pr[2 * (size_t)i + 1];
    const float cc[3] = {c.x, c.y, c.z}, nn[3] = {n.x, n.y, n.z};
    for (int k = 0; k < 3; ++k) { // the disc's own extent along axis k (as the BVH's boxes)
      const float e = c.w * sqrtf(fmaxf(0.f, 1.f - nn[k] * nn[k])) * 1.0001f;
      lo[k] = cc[k] - e;
      hi[k] = cc[k] + e;
    }
  } else {
    const float4 a = pr[4 * (size_t)i], e1 = pr[4 * (size_t)i + 1], e2 = pr[4 * (size_t)i + 2];
    const float v0[3] = {a.x, a.y, a.z}, v1[3] = {a.x - e1.x, a.y - e1.y, a.z - e1.z}, v2[3] = {a.x + e2.x, a.y + e2.y, a.z + e2.z};
    for (int k = 0; k < 3; ++k) {
      lo[k] = fminf(v0[k], fminf(v1[k], v2[k]));
      hi[k] = fmaxf(v0[k], fmaxf(v1[k], v2[k]));
    }
  }
}

__global__ void relief_field_kernel(ReliefParams q) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= q.n)
    return;
  float lo[3], hi[3];
  relief_prim_box(q, i, lo, hi);
  // (the pad — 1e-5 of the largest coordinate — is far above the rounding of a ray's position and of the tile walk: a
  //  point of a primitive that the walk files under the neighbouring tile is still inside that tile's range)
  const unsigned zl = f2ord(lo[q.ax] - q.pad), zh = f2ord(hi[q.ax] + q.pad);
  const int ix0 = min(max((int)floorf((lo[q.a1] - q.pad - q.lo1) * q.invTile), 0), q.nx - 1);
  const int ix1 = min(max((int)floorf((hi[q.a1] + q.pad - q.lo1) * q.invTile), 0), q.nx - 1);
  int iy0 = 0, iy1 = 0;
  if (q.ny > 1) {
    iy0 = min(max((int)floorf((lo[q.a2] - q.pad - q.lo2) * q.invTile), 0), q.ny - 1);
    iy1 = min(max((int)floorf((hi[q.a2] + q.pad - q.lo2) * q.invTile), 0), q.ny - 1);
  }
  for (int iy = iy0; iy <= iy1; ++iy)
    for (int ix = ix0; ix <= ix1; ++ix) {
      atomicMin(&q.rawLo[iy * q.nx + ix], zl);
      atomicMax(&q.rawHi[iy * q.nx + ix], zh);
    }
}

// one thread per COARSE tile: its k x k fine tiles -> {lo, hi} floats, the coarse entry and the statistics
__global__ void relief_finish_kernel(ReliefParams q) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= q.cnx * q.cny)
    return;
  const int cx = t % q.cnx, cy = t / q.cnx;
  float mlo = 3.0e38f, mhi = -3.0e38f, thick = 0.f;
  unsigned filled = 0;
  for (int dy = 0; dy < q.k; ++dy)
    for (int dx = 0; dx < q.k; ++dx) {
      const int ix = cx * q.k + dx, iy = cy * q.k + dy;
      if (ix >= q.nx || iy >= q.ny)
        continue;
      const unsigned ul = q.rawLo[iy * q.nx + ix], uh = q.rawHi[iy * q.nx + ix];
      float2 f = make_float2(3.0e38f, -3.0e38f); // (a tile nothing reaches into: no height overlaps it)
      if (uh != 0u) {
        f = make_float2(ord2f(ul), ord2f(uh));
        mlo = fminf(mlo, f.x);
        mhi = fmaxf(mhi, f.y);
        thick = fmaxf(thick, f.y - f.x);
        ++filled;
      }
      reinterpret_cast<float2 *>(q.fine)[iy * q.nx + ix] = f;
    }
  reinterpret_cast<float2 *>(q.coarse)[t] = filled ? make_float2(0.5f * (mlo + mhi), thick) : make_float2(q.emptyMid, 0.f);
  if (filled) {
    atomicAdd(&q.stats[0], 1u);
    atomicAdd(&q.stats[1], (unsigned)(4096.f * thick * thick / (thick * thick + q.travel * q.travel)));
  }
}

hipError_t launch_relief_field(const ReliefParams &q, hipStream_t st) {
  hipError_t e = hipMemsetAsync(q.rawLo, 0xFF, (size_t)q.nx * q.ny * 4, st);
  if (e == hipSuccess)
    e = hipMemsetAsync(q.rawHi, 0, (size_t)q.nx * q.ny * 4, st);
  if (e == hipSuccess)
    e = hipMemsetAsync(q.stats, 0, 2 * 4, st);
  if (e != hipSuccess)
    return e;
  if (q.n)
    hipLaunchKernelGGL(relief_field_kernel, dim3((q.n + 255) / 256), dim3(256), 0, st, q);
  hipLaunchKernelGGL(relief_finish_kernel, dim3((q.cnx * q.cny + 255) / 256), dim3(256), 0, st, q);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// uniform disks: one normal and one radius for the whole cloud (a disk cloud made from a planar level set), compared as
// 32-bit words (a -0 is not a +0, a NaN equals itself): where it holds, record 0's four words stand for every record's.
// In the same pass, for the planar variant (vr_planar_disks.hpp): per coordinate, whether every centre carries record
// 0's word in it, and whether every centre coordinate is finite.  out: VR_UNIFORM_WORDS words —
// [0] a normal or radius differs, [1..4] record 0's n.x, n.y, n.z, radius, [5..7] a centre's x / y / z differs from
// record 0's, [8] a centre coordinate is not finite, [9..11] record 0's c.x, c.y, c.z
// ---------------------------------------------------------------------------
__global__ void uniform_disks_kernel(const uint4 *__restrict__ recs, unsigned n, unsigned *out) {
  const uint4 c0 = recs[0], n0 = recs[1];
  bool same = true, sameX = true, sameY = true, sameZ = true, finite = true;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint4 c = recs[2 * (size_t)i], nn = recs[2 * (size_t)i + 1];
    same = same && nn.x == n0.x && nn.y == n0.y && nn.z == n0.z && c.w == c0.w;
    sameX = sameX && c.x == c0.x;
    sameY = sameY && c.y == c0.y;
    sameZ = sameZ && c.z == c0.z;
    // (an all-ones exponent: an infinity or a NaN)
    finite = finite && (c.x & 0x7F800000u) != 0x7F800000u && (c.y & 0x7F800000u) != 0x7F800000u && (c.z & 0x7F800000u) != 0x7F800000u;
  }
  if (!same)
    out[0] = 1u; // (every writer writes the same word)
  if (!sameX)
    out[5] = 1u;
  if (!sameY)
    out[6] = 1u;
  if (!sameZ)
    out[7] = 1u;
  if (!finite)
    out[8] = 1u;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    out[1] = n0.x;
    out[2] = n0.y;
    out[3] = n0.z;
    out[4] = c0.w;
    out[9] = c0.x;
    out[10] = c0.y;
    out[11] = c0.z;
  }
}

hipError_t launch_uniform_disks(const float *prims, unsigned n, unsigned *out, hipStream_t st) {
  hipError_t e = hipMemsetAsync(out, 0, VR_UNIFORM_WORDS * 4, st);
  if (e != hipSuccess || n == 0)
    return e;
  const unsigned grid = (unsigned)((n + 255u) / 256u < 1024u ? (n + 255u) / 256u : 1024u);
  hipLaunchKernelGGL(uniform_disks_kernel, dim3(grid), dim3(256), 0, st, reinterpret_cast<const uint4 *>(prims), n, out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// lattice table of a planar cloud (vr_planar_lattice.hpp): one pass over the packed records, in leaf order, validates and
// fills.  Every disk claims the word of its lattice point with a compare-and-swap on the empty word; a centre off the
// lattice (lattice_cell_of) raises bit 0 of the flag word, a second disk at one point bit 1.  Every index is formed by
// lattice_cell_of, which hands out nothing outside n1 x n2.
// ---------------------------------------------------------------------------
__global__ void lattice_table_kernel(const float4 *__restrict__ recs, unsigned n, int b1, int b2, float phase1, float phase2,
                                     float invDelta, int n1, int n2, unsigned *table, unsigned *flag) {
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float4 c = recs[2 * (size_t)i];
    const float u = b1 == 0 ? c.x : c.y, v = b2 == 2 ? c.z : c.y; // (b1 < b2: planar_in_plane_axes)
    int ci, cj;
    const bool on1 = lattice_cell_of(u, phase1, invDelta, n1, ci), on2 = lattice_cell_of(v, phase2, invDelta, n2, cj);
    if (!(on1 && on2))
      atomicOr(flag, 1u);
    else if (atomicCAS(&table[(size_t)cj * (size_t)n1 + (size_t)ci], VR_LATTICE_EMPTY, i) != VR_LATTICE_EMPTY)
      atomicOr(flag, 2u);
  }
}

hipError_t launch_lattice_table(const float *prims, unsigned n, int b1, int b2, float phase1, float phase2, float invDelta,
                                int n1, int n2, unsigned *table, hipStream_t st) {
  if (n1 < 1 || n2 < 1 || n == 0)
    return hipErrorInvalidValue;
  const size_t cells = (size_t)n1 * (size_t)n2;
  hipError_t e = hipMemsetAsync(table, 0xFF, cells * 4, st); // (VR_LATTICE_EMPTY in every word)
  if (e == hipSuccess)
    e = hipMemsetAsync(table + cells, 0, 4, st);
  if (e != hipSuccess)
    return e;
  const unsigned grid = (unsigned)((n + 255u) / 256u < 1024u ? (n + 255u) / 256u : 1024u);
  hipLaunchKernelGGL(lattice_table_kernel, dim3(grid), dim3(256), 0, st, reinterpret_cast<const float4 *>(prims), n, b1, b2,
                     phase1, phase2, invDelta, n1, n2, table, table + cells);
  return hipGetLastError();
}

} // namespace vr
