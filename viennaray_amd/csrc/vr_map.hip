// vr_map.hip — per-primitive values mapped to the caller's points (vr_map_to_points_device): one walk of the resident
// float4 link/escape nodes per query point serves both the weighted mean over the primitive centres within the radius
// and the nearest-centre fallback.  A translation unit of its own: nothing an apply() runs is in it.
//
//   map_keys_kernel     63-bit Morton key of every query point in the scene box (the sort that makes neighbouring lanes
//                       walk alike; vr_sort.hip: launch_sort_pairs)
//   map_points_kernel   the walk.  d = |p - c_j|, in range iff d < R, w = (1 - d / R) * max(0, n_j . m^), out = sum w f /
//                       sum w, or f of the nearest centre (lowest original id on a tie) where the sum of weights is not
//                       positive.  The sums run in the order of the walk.
//
// The centres: a disk's is the caller's point — the packed record's centre carries the same words (disk4_kernel; z is 0
// in 2-D, where z is not looked at) — a triangle's is ((v0 + v1) + v2) * (1.f / 3.f) per component, from the resident
// vertices.  The packed records (leaf order) also hold the normal and the original id.
//
// Pruning.  A node is skipped when the squared distance from the query to its box exceeds max(R^2, best^2), best the
// nearest centre distance so far.  The box distance is a lower bound of the distance to every centre below the node:
//  * the float4 boxes are the primitives' boxes and their unions, unquantised and PADDED outwards by morton_kernel
//    (4e-6 of the scene's largest coordinate) — a disk's box is symmetric about its centre, a triangle's holds its
//    vertices, and the rounding of the float32 centroid (three roundings, below 4e-7 of the coordinate) stays inside the
//    padding;
//  * both distances are computed by the same float operations in the same order (differences, squares, (x + y) + z,
//    -ffp-contract=off), and every one of them is monotone: with lo <= c <= hi the box's figure cannot come out above
//    the centre's.
// R^2 is widened by two units in the last place for the bound, so that "d < R" is decided on the rounded d alone.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "vr_kernels.hpp"
#include "vr_setup_common.hpp"
#include "vr_types.hpp"

namespace vr {

__device__ __forceinline__ u64 map_spread21(u64 v) {
  v &= 0x1FFFFFull;
  v = (v | v << 32) & 0x1F00000000FFFFull;
  v = (v | v << 16) & 0x1F0000FF0000FFull;
  v = (v | v << 8) & 0x100F00F00F00F00Full;
  v = (v | v << 4) & 0x10C30C30C30C30C3ull;
  v = (v | v << 2) & 0x1249249249249249ull;
  return v;
}

constexpr unsigned MAP_BLOCK = 256;
constexpr unsigned MAP_MAX_BLOCKS = 1u << 20; // grid-stride beyond that

struct MapBox {
  float lo[3], inv[3]; // scene box: low corner, 2097151 / extent (0 where the box is flat)
};

__global__ __launch_bounds__(MAP_BLOCK) void map_keys_kernel(const float *pts, unsigned m, unsigned ld, int D, MapBox box,
                                                             u64 *keys, unsigned *vals) {
  for (u64 t = (u64)blockIdx.x * MAP_BLOCK + threadIdx.x; t < m; t += (u64)gridDim.x * MAP_BLOCK) {
    const float *p = pts + t * ld;
    u64 q[3] = {0, 0, 0};
    for (int k = 0; k < D; ++k) {
      float c = (p[k] - box.lo[k]) * box.inv[k];
      c = c >= 0.f ? c : 0.f; // (a NaN: cell 0 — any key will do for a point that is answered without a walk)
      c = c <= 2097151.0f ? c : 2097151.0f;
      q[k] = (u64)c;
    }
    keys[t] = (map_spread21(q[0]) << 2) | (map_spread21(q[1]) << 1) | map_spread21(q[2]);
    vals[t] = (unsigned)t;
  }
}

struct MapParams {
  const float4 *nodes, *prims; // the resident build: 2 float4 per node; 2 (disks) / 4 (triangles) float4 per primitive
  const float *verts;          // triangles
  const uint32_t *tris;
  const float *values, *pts, *nrm; // nrm: nullptr = no normal gate
  const unsigned *perm;            // nullptr: query t is row t; else row perm[t]
  float *out;
  unsigned long long *visits; // VR_DIAG: node visits of all queries
  unsigned m, ld;
  float radius;
};

// squared distance from the query to a node's box: per axis max(lo - p, p - hi, 0), written so that a NaN stays a NaN
// (and fails every `<=` it meets)
template <int D> __device__ __forceinline__ float map_box_d2(const float4 &a, const float4 &b, float px, float py, float pz) {
  float dx = a.x - px, dy = a.y - py, dz = 0.f;
  const float ux = px - b.x, uy = py - b.y;
  dx = ux > dx ? ux : dx;
  dy = uy > dy ? uy : dy;
  dx = dx < 0.f ? 0.f : dx;
  dy = dy < 0.f ? 0.f : dy;
  if (D == 3) {
    dz = a.z - pz;
    const float uz = pz - b.z;
    dz = uz > dz ? uz : dz;
    dz = dz < 0.f ? 0.f : dz;
  }
  return (dx * dx + dy * dy) + dz * dz;
}

// the primitive at leaf position q: its original id, and the squared distance from the query to its centre
template <int GEO, int D>
__device__ __forceinline__ float map_centre_d2(const MapParams &p, size_t q, float px, float py, float pz, unsigned &o) {
  float cx, cy, cz;
  if (GEO == 0) {
    const float4 c4 = p.prims[2 * q];
    cx = c4.x, cy = c4.y, cz = c4.z;
    o = __float_as_uint(p.prims[2 * q + 1].w);
  } else {
    o = __float_as_uint(p.prims[4 * q].w);
    const float *v0 = p.verts + 3 * (size_t)p.tris[3 * (size_t)o];
    const float *v1 = p.verts + 3 * (size_t)p.tris[3 * (size_t)o + 1];
    const float *v2 = p.verts + 3 * (size_t)p.tris[3 * (size_t)o + 2];
    cx = ((v0[0] + v1[0]) + v2[0]) * (1.f / 3.f);
    cy = ((v0[1] + v1[1]) + v2[1]) * (1.f / 3.f);
    cz = D == 3 ? ((v0[2] + v1[2]) + v2[2]) * (1.f / 3.f) : 0.f;
  }
  const float ex = px - cx, ey = py - cy, ez = D == 3 ? pz - cz : 0.f;
  return (ex * ex + ey * ey) + ez * ez;
}

template <int GEO, int D>
__global__ __launch_bounds__(MAP_BLOCK) void map_points_kernel(MapParams p) {
  const float R = p.radius, R2 = R * R;
  const float R2bound = R2 + R2 * 2.4e-7f; // (>= every d^2 whose rounded root is below R)
  const float INF = __int_as_float(0x7F800000), QNAN = __int_as_float(0x7FC00000);
#ifdef VR_DIAG
  unsigned long long visits = 0;
#endif
  for (u64 t = (u64)blockIdx.x * MAP_BLOCK + threadIdx.x; t < p.m; t += (u64)gridDim.x * MAP_BLOCK) {
    const size_t i = p.perm ? p.perm[t] : (size_t)t;
    const float px = p.pts[i * p.ld], py = p.pts[i * p.ld + 1], pz = D == 3 ? p.pts[i * p.ld + 2] : 0.f;
    if (!(fabsf(px) <= FLT_MAX && fabsf(py) <= FLT_MAX && fabsf(pz) <= FLT_MAX)) { // NaN or +-inf: no walk
      p.out[i] = QNAN;
      continue;
    }
    float mx = 0.f, my = 0.f, mz = 0.f;
    if (p.nrm) {
      mx = p.nrm[i * p.ld];
      my = p.nrm[i * p.ld + 1];
      mz = D == 3 ? p.nrm[i * p.ld + 2] : 0.f;
      const float len = sqrtf((mx * mx + my * my) + mz * mz);
      mx /= len;
      my /= len;
      mz /= len;
    }
    float best2 = INF, sw = 0.f, sv = 0.f;
    unsigned bestId = 0xFFFFFFFFu;
    // The seed of `best`: one descent to the leaf whose boxes lie nearest on the way down.  A centre distance found
    // there is an upper bound of the nearest one, so the walk below starts with a bound near its final value.  (The
    // walk visits subtrees in the tree's order, not nearest first: started with best = inf it carries the distance of
    // the first leaf it meets, anywhere in the scene, through everything in between — measured, 10^6 sorted queries on
    // 10^6 disks: 50 ms without the seed, 1 ms with it.)  The seed's leaf is met again by the walk, which alone sums.
    {
      float4 a = p.nodes[0];
      while (!(__float_as_uint(a.w) & VR_LEAF)) {
        const unsigned c0 = __float_as_uint(a.w);
        const float4 a0 = p.nodes[2 * (size_t)c0], b0 = p.nodes[2 * (size_t)c0 + 1];
        const unsigned c1 = __float_as_uint(b0.w); // (the first child's escape is its sibling)
        a = a0;
        if (c1 != VR_END) {
          const float4 a1 = p.nodes[2 * (size_t)c1], b1 = p.nodes[2 * (size_t)c1 + 1];
          if (map_box_d2<D>(a1, b1, px, py, pz) < map_box_d2<D>(a0, b0, px, py, pz))
            a = a1;
        }
#ifdef VR_DIAG
        visits += 2;
#endif
      }
      const unsigned link = __float_as_uint(a.w);
      const unsigned first = link & VR_LEAF_FIRST_MASK, cnt = (link >> 27) & 15u;
      for (unsigned k = 0; k < cnt; ++k) {
        unsigned o;
        const float d2 = map_centre_d2<GEO, D>(p, first + k, px, py, pz, o);
        if (d2 < best2 || (d2 == best2 && o < bestId)) {
          best2 = d2;
          bestId = o;
        }
      }
    }
    unsigned node = 0;
    while (node != VR_END) {
      const float4 a = p.nodes[2 * (size_t)node], b = p.nodes[2 * (size_t)node + 1];
      const unsigned link = __float_as_uint(a.w), esc = __float_as_uint(b.w);
#ifdef VR_DIAG
      ++visits;
#endif
      const float bd2 = map_box_d2<D>(a, b, px, py, pz);
      const float bound = R2bound > best2 ? R2bound : best2;
      if (!(bd2 <= bound)) { // too far (or not a number): the subtree is skipped
        node = esc;
        continue;
      }
      if (!(link & VR_LEAF)) {
        node = link;
        continue;
      }
      const unsigned first = link & VR_LEAF_FIRST_MASK, cnt = (link >> 27) & 15u;
      for (unsigned k = 0; k < cnt; ++k) {
        const size_t q = first + k;
        unsigned o;
        const float d2 = map_centre_d2<GEO, D>(p, q, px, py, pz, o);
        if (d2 < best2 || (d2 == best2 && o < bestId)) {
          best2 = d2;
          bestId = o;
        }
        if (d2 <= R2bound) {
          const float d = sqrtf(d2);
          if (d < R) {
            float w = 1.f - d / R;
            if (p.nrm) {
              float nx, ny, nz;
              if (GEO == 0) {
                const float4 n4 = p.prims[2 * q + 1];
                nx = n4.x, ny = n4.y, nz = n4.z;
              } else {
                nx = p.prims[4 * q + 1].w;
                ny = p.prims[4 * q + 2].w;
                nz = p.prims[4 * q + 3].w;
              }
              float g = D == 3 ? (nx * mx + ny * my) + nz * mz : nx * mx + ny * my;
              g = g > 0.f ? g : 0.f; // (a NaN gate closes)
              w *= g;
            }
            sw += w;
            sv += w * p.values[o];
          }
        }
      }
      node = esc;
    }
    float r = QNAN; // (no primitive at all)
    if (sw > 0.f)
      r = sv / sw;
    else if (bestId != 0xFFFFFFFFu)
      r = p.values[bestId];
    p.out[i] = r;
  }
#ifdef VR_DIAG
  if (p.visits && visits)
    atomicAdd(p.visits, visits);
#endif
}

static unsigned map_grid(unsigned m) {
  const u64 blocks = ((u64)m + MAP_BLOCK - 1) / MAP_BLOCK;
  return (unsigned)(blocks < MAP_MAX_BLOCKS ? blocks : MAP_MAX_BLOCKS);
}

hipError_t launch_map_keys(const float *pts, unsigned m, unsigned ld, int D, const float *sceneLo, const float *sceneHi,
                           unsigned long long *keys, unsigned *vals, hipStream_t st) {
  if (m == 0)
    return hipSuccess;
  MapBox box;
  for (int k = 0; k < 3; ++k) {
    const float ext = sceneHi[k] - sceneLo[k];
    box.lo[k] = sceneLo[k];
    box.inv[k] = ext > 0.f ? 2097151.0f / ext : 0.f;
  }
  hipLaunchKernelGGL(map_keys_kernel, dim3(map_grid(m)), dim3(MAP_BLOCK), 0, st, pts, m, ld, D, box, keys, vals);
  return hipGetLastError();
}

hipError_t launch_map_points(const SetupParams &s, const float *values, const float *pts, const float *nrm, unsigned m,
                             unsigned ld, float radius, const unsigned *perm, float *out, unsigned long long *visits,
                             hipStream_t st) {
  if (m == 0)
    return hipSuccess;
  MapParams p{};
  p.nodes = reinterpret_cast<const float4 *>(s.nodes);
  p.prims = reinterpret_cast<const float4 *>(s.prims);
  p.verts = s.verts;
  p.tris = s.tris;
  p.values = values;
  p.pts = pts;
  p.nrm = nrm;
  p.perm = perm;
  p.out = out;
  p.visits = visits;
  p.m = m;
  p.ld = ld;
  p.radius = radius;
  const dim3 g(map_grid(m)), b(MAP_BLOCK);
  if (s.geo == 0) {
    if (s.D == 2)
      hipLaunchKernelGGL((map_points_kernel<0, 2>), g, b, 0, st, p);
    else
      hipLaunchKernelGGL((map_points_kernel<0, 3>), g, b, 0, st, p);
  } else {
    if (s.D == 2)
      hipLaunchKernelGGL((map_points_kernel<1, 2>), g, b, 0, st, p);
    else
      hipLaunchKernelGGL((map_points_kernel<1, 3>), g, b, 0, st, p);
  }
  return hipGetLastError();
}

} // namespace vr
