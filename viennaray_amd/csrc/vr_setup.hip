// vr_setup.hip — device-side scene setup: LBVH build and disk-neighbourhood CSR.
//
// The reference builds its acceleration structure inside the timed region
// (rtcJoinCommitScene, rayTraceKernel.hpp:91) and its point
// neighbourhood at setGeometry (rayGeometryDisk.hpp:191-192, recursive host
// vectors).  Here both are HIP kernels:
//
//   prim_box_kernel     primitive AABBs (oriented-disc extents r*sqrt(1-n_k^2),
//                       triangle min/max) + scene bounds (ordered-int atomics)
//   morton_kernel       63-bit Morton code of each box centre
//   radix sort          LSD, 8-bit digits, one wavefront per 1024-key tile,
//                       ballot-based stable ranking (no LDS scatter buffers)
//   karras_kernel       binary radix tree over the sorted codes (Karras 2012)
//   fit_kernel          bottom-up AABB fit with arrival counters
//   fit_kernel          ... + emitted subtree sizes and the source-side-first child order
//   finalize_kernel     traversal nodes {lo,link}{hi,escape} in pre-order: ranges of
//                       <= leafMax primitives collapse into leaves
//   quantize_nodes      16-byte nodes (16-bit conservative boxes) for per-lane traversal
//   pack_*_kernel       primitive records in leaf order
//   nb_count / nb_fill  neighbourhood = stackless BVH range query around every
//                       disc centre (per-axis |d| <= dist and |d|^2 <= dist^2,
//                       rayPointNeighborhood.hpp:287-298), written as CSR of leaf
//                       positions
#include <hip/hip_runtime.h>

#include <cfloat>

#include "vr_area.hpp"
#include "vr_kernels.hpp"
#include "vr_types.hpp"

namespace vr {

typedef unsigned long long u64;

// ---------------------------------------------------------------------------
// float <-> order-preserving uint (for atomicMin/Max on floats)
// ---------------------------------------------------------------------------
__device__ __forceinline__ unsigned f2ord(float f) {
  unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline float ord2f(unsigned u) {
  unsigned v = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
#ifdef __HIP_DEVICE_COMPILE__
  return __uint_as_float(v);
#else
  float f;
  __builtin_memcpy(&f, &v, 4);
  return f;
#endif
}

// bounds[0..2] = min (ordered), bounds[3..5] = max (ordered)
__global__ void prim_box_kernel(SetupParams s) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  if (i < s.n) {
    if (s.geo == 0) {
      const float4 d = reinterpret_cast<const float4 *>(s.disk4)[i];
      float nx = s.normal3[3 * (size_t)i], ny = s.normal3[3 * (size_t)i + 1], nz = s.normal3[3 * (size_t)i + 2];
      const float nn = sqrtf((nx * nx + ny * ny) + nz * nz);
      if (nn > 0.f) {
        nx /= nn;
        ny /= nn;
        nz /= nn;
      }
      const float c[3] = {d.x, d.y, d.z}, nv[3] = {nx, ny, nz};
      for (int k = 0; k < 3; ++k) {
        const float h = d.w * sqrtf(fmaxf(0.f, 1.f - nv[k] * nv[k])) * 1.0001f;
        lo[k] = c[k] - h;
        hi[k] = c[k] + h;
      }
    } else {
      const unsigned a = s.tris[3 * (size_t)i], b = s.tris[3 * (size_t)i + 1], c = s.tris[3 * (size_t)i + 2];
      for (int k = 0; k < 3; ++k) {
        const float v0 = s.verts[3 * (size_t)a + k], v1 = s.verts[3 * (size_t)b + k], v2 = s.verts[3 * (size_t)c + k];
        lo[k] = fminf(v0, fminf(v1, v2));
        hi[k] = fmaxf(v0, fmaxf(v1, v2));
      }
    }
    float *b = s.box + 6 * (size_t)i;
    for (int k = 0; k < 3; ++k) {
      b[k] = lo[k];
      b[3 + k] = hi[k];
    }
  }
  // wave reduce, block reduce through LDS, then six atomics per BLOCK (one per wave made
  // 10^5 same-address atomics on a 10^6-disk scene: 1 ms)
  __shared__ float red[6][4];
  for (int k = 0; k < 3; ++k) {
    float a = lo[k], b = hi[k];
    for (int off = 32; off > 0; off >>= 1) {
      a = fminf(a, __shfl_down(a, off, 64));
      b = fmaxf(b, __shfl_down(b, off, 64));
    }
    if ((threadIdx.x & 63) == 0) {
      red[k][threadIdx.x >> 6] = a;
      red[3 + k][threadIdx.x >> 6] = b;
    }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int k = threadIdx.x;
    const unsigned nw = (blockDim.x + 63) >> 6;
    float v = red[k][0];
    for (unsigned w = 1; w < nw; ++w)
      v = k < 3 ? fminf(v, red[k][w]) : fmaxf(v, red[k][w]);
    if (k < 3)
      atomicMin(&s.bounds[k], f2ord(v));
    else
      atomicMax(&s.bounds[k], f2ord(v));
  }
}

__device__ __forceinline__ u64 spread21(u64 v) {
  v &= 0x1FFFFFull;
  v = (v | v << 32) & 0x1F00000000FFFFull;
  v = (v | v << 16) & 0x1F0000FF0000FFull;
  v = (v | v << 8) & 0x100F00F00F00F00Full;
  v = (v | v << 4) & 0x10C30C30C30C30C3ull;
  v = (v | v << 2) & 0x1249249249249249ull;
  return v;
}

// pads the boxes (more than the rounding of the slab test) and computes codes
__global__ void morton_kernel(SetupParams s) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= s.n)
    return;
  float slo[3], shi[3], scale = 0.f;
  for (int k = 0; k < 3; ++k) {
    slo[k] = ord2f(s.bounds[k]);
    shi[k] = ord2f(s.bounds[3 + k]);
    scale = fmaxf(scale, fmaxf(fabsf(slo[k]), fabsf(shi[k])));
  }
  const float pad = 4e-6f * fmaxf(scale, 1e-3f);
  float *b = s.box + 6 * (size_t)i;
  u64 q[3];
  // The grid's cell has the proportions of the scene box — but only up to mortonAniso : 1.  Scaled freely axis by
  // axis, a thin sheet (1000 x 1000 cells wide, one cell of relief) spends every third bit of the code on its relief:
  // the tree cuts it into contour bands whose boxes overlap everywhere in plan (measured on a 10^6-disk rippled sheet:
  // 110 pair visits and 18 leaf tests per ray, 33 ms for 3e7 rays; 9.7 ms with bounded proportions).  Cubes throughout
  // cost the 60 x 60 x 30 trench 5 %: cells twice as fine along the short (source) axis serve it better.
  const float extMax = fmaxf(fmaxf(shi[0] - slo[0], shi[1] - slo[1]), shi[2] - slo[2]);
  for (int k = 0; k < 3; ++k) {
    const float ext = fmaxf(shi[k] - slo[k], extMax / s.mortonAniso);
    const float inv = ext > 0.f ? 2097151.0f / ext : 0.f;
    float c = (0.5f * (b[k] + b[3 + k]) - slo[k]) * inv;
    c = fminf(fmaxf(c, 0.f), 2097151.0f);
    q[k] = (u64)c;
    b[k] -= pad;
    b[3 + k] += pad;
  }
  s.keysA[i] = (spread21(q[0]) << 2) | (spread21(q[1]) << 1) | spread21(q[2]);
  s.valsA[i] = i;
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

// ---------------------------------------------------------------------------
// Karras binary radix tree
// ---------------------------------------------------------------------------
constexpr unsigned CHILD_LEAF = 0x80000000u; // child is the singleton leaf of that sorted position

__device__ __forceinline__ int delta(const u64 *code, int n, int i, int j) {
  if (j < 0 || j >= n)
    return -1;
  const u64 a = code[i], b = code[j];
  if (a == b)
    return 64 + __clz((unsigned)i ^ (unsigned)j);
  return __clzll((long long)(a ^ b));
}

__global__ void karras_kernel(SetupParams s) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int n = (int)s.n;
  if (i >= n - 1)
    return;
  const u64 *code = s.keysA;
  const int d = (delta(code, n, i, i + 1) - delta(code, n, i, i - 1)) >= 0 ? 1 : -1;
  const int dmin = delta(code, n, i, i - d);
  int lmax = 2;
  while (delta(code, n, i, i + lmax * d) > dmin)
    lmax *= 2;
  int l = 0;
  for (int t = lmax / 2; t >= 1; t /= 2)
    if (delta(code, n, i, i + (l + t) * d) > dmin)
      l += t;
  const int j = i + l * d;
  const int dnode = delta(code, n, i, j);
  int sp = 0;
  int t = l;
  do {
    t = (t + 1) >> 1;
    if (delta(code, n, i, i + (sp + t) * d) > dnode)
      sp += t;
  } while (t > 1);
  const int gamma = i + sp * d + (d < 0 ? d : 0);
  const int lo = i < j ? i : j, hi = i < j ? j : i;
  const unsigned left = (lo == gamma) ? (CHILD_LEAF | (unsigned)gamma) : (unsigned)gamma;
  const unsigned right = (hi == gamma + 1) ? (CHILD_LEAF | (unsigned)(gamma + 1)) : (unsigned)(gamma + 1);
  s.rangeLo[i] = (unsigned)lo;
  s.rangeHi[i] = (unsigned)hi;
  s.childL[i] = left;
  s.childR[i] = right;
  // parent links; bit 31 of the stored parent marks "I am the right child"
  if (left & CHILD_LEAF)
    s.parentLeaf[left & ~CHILD_LEAF] = (unsigned)i;
  else
    s.parentInt[left] = (unsigned)i;
  if (right & CHILD_LEAF)
    s.parentLeaf[right & ~CHILD_LEAF] = (unsigned)i | 0x80000000u;
  else
    s.parentInt[right] = (unsigned)i | 0x80000000u;
}

// bottom-up AABB fit: thread = sorted position; the second arriver at a node fits it.
// The same pass computes what the pre-order layout needs: the number of traversal
// nodes each subtree EMITS (a range of <= leafMax primitives collapses into one leaf)
// and which child the traversal should visit first (bit 31): the one whose box centre
// lies closer to the source plane, so that primary rays meet their first hit early
// and the escape-link walk culls everything behind it.
__global__ void fit_kernel(SetupParams s) {
  const unsigned q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= s.n || s.n < 2)
    return;
  unsigned p = s.parentLeaf[q] & 0x7FFFFFFFu;
  for (;;) {
    // Hand-over between the two arrivers of a node.  Everything a fitter publishes (box, subtree
    // size) is written with agent-scope atomic stores (`global_store ... sc1`: write-through, not
    // kept in this XCD's L2) and read with agent-scope atomic loads (`sc1`: served below the
    // reader's L1), which are coherent across the XCDs by themselves; what remains is ORDER: every
    // such store of this lane must have been acknowledged before the arrival counter is bumped.
    // That is the explicit `s_waitcnt vmcnt(0)` below (inline asm: no compiler pass can drop or
    // move it; tests/test_isa_contracts.py checks the emitted ISA).  It replaces an agent-scope
    // release fence, whose `buffer_wbl2` write-back of the whole L2 made this kernel 3.0 ms instead
    // of 0.2 ms on 10^6 disks and which these sc1 stores do not need.  s.strictFence selects the
    // textbook form (agent-scope release / acquire fences) instead: build_scene() re-runs the fit
    // that way should launch_bvh_check ever report a violation.
    if (s.strictFence)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned arrived = __hip_atomic_fetch_add(&s.arrive[p], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (arrived == 0u)
      return; // first arriver: the sibling will come
    if (s.strictFence)
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    const unsigned L = s.childL[p], R = s.childR[p];
    const float *a = (L & CHILD_LEAF) ? s.sbox + 6 * (size_t)(L & ~CHILD_LEAF) : s.nodeBox + 6 * (size_t)L;
    const float *b = (R & CHILD_LEAF) ? s.sbox + 6 * (size_t)(R & ~CHILD_LEAF) : s.nodeBox + 6 * (size_t)R;
    float *o = s.nodeBox + 6 * (size_t)p;
    float ba[6], bb[6];
    for (int k = 0; k < 6; ++k) {
      ba[k] = __hip_atomic_load(&a[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      bb[k] = __hip_atomic_load(&b[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    for (int k = 0; k < 3; ++k) {
      __hip_atomic_store(&o[k], fminf(ba[k], bb[k]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(&o[3 + k], fmaxf(ba[3 + k], bb[3 + k]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const unsigned sl =
        (L & CHILD_LEAF) ? 1u : (__hip_atomic_load(&s.subSize[L], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 0x7FFFFFFFu);
    const unsigned sr =
        (R & CHILD_LEAF) ? 1u : (__hip_atomic_load(&s.subSize[R], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 0x7FFFFFFFu);
    const unsigned cnt = s.rangeHi[p] - s.rangeLo[p] + 1u;
    const unsigned size = cnt <= s.leafMax ? 1u : 1u + sl + sr;
    const int ax = s.orderAxis;
    const bool rightFirst = s.orderSign * ((bb[ax] + bb[3 + ax]) - (ba[ax] + ba[3 + ax])) > 0.f;
    __hip_atomic_store(&s.subSize[p], size | (rightFirst ? 0x80000000u : 0u), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    if (p == 0)
      return;
    p = s.parentInt[p] & 0x7FFFFFFFu;
  }
}

// Traversal nodes, written twice from the (child-ordered, leaf-collapsed) tree:
//  * s.nodes   : build numbering (internal i -> i, singleton leaf of sorted position q ->
//                n-1+q): the two children of a node are NEIGHBOURS in memory, which is what
//                the packet traversal's scalar fetches like (a missed first child is
//                followed by its sibling, same 64-byte line).  Explicit link + escape.
//  * s.nodesPre: PRE-ORDER: the first child of an internal node is the next node, the
//                escape of any node is the node after its subtree.  Source of the 16-byte
//                nodes of the per-lane walk, which keep ONE link word thanks to that.
// Thread t = node of the build numbering; a node below a collapsed range is not emitted.
// One walk to the root yields both the pre-order index (every ancestor contributes 1,
// plus the size of the sibling subtree where the path is the second child) and the
// escape in build numbering (sibling of the nearest ancestor-or-self that is a first
// child).
__device__ __forceinline__ unsigned sub_size(const SetupParams &s, unsigned child) {
  return (child & CHILD_LEAF) ? 1u : (s.subSize[child] & 0x7FFFFFFFu);
}
__device__ __forceinline__ unsigned node_of_child(const SetupParams &s, unsigned c) {
  return (c & CHILD_LEAF) ? (s.n - 1u) + (c & ~CHILD_LEAF) : c;
}

__global__ void finalize_kernel(SetupParams s) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned n = s.n;
  float4 *nodes = reinterpret_cast<float4 *>(s.nodes);
  float4 *nodesPre = reinterpret_cast<float4 *>(s.nodesPre);
  if (n == 1) {
    if (t == 0) {
      const float *b = s.sbox;
      const float4 a0 = make_float4(b[0], b[1], b[2], __uint_as_float(VR_LEAF | (1u << 27) | 0u));
      const float4 a1 = make_float4(b[3], b[4], b[5], __uint_as_float(VR_END));
      nodes[0] = nodesPre[0] = a0;
      nodes[1] = nodesPre[1] = a1;
      s.subSize[0] = 1u;
    }
    return;
  }
  if (t >= 2 * n - 1)
    return;
  const bool internal = t < n - 1;
  const unsigned q = internal ? 0u : t - (n - 1);
  unsigned pw = 0; // parent index | "I am the right child"
  bool haveParent = true;
  if (internal) {
    if (t == 0)
      haveParent = false;
    else
      pw = s.parentInt[t];
  } else {
    pw = s.parentLeaf[q];
  }
  if (haveParent) { // not emitted below a collapsed range (ancestors' ranges only grow)
    const unsigned pp = pw & 0x7FFFFFFFu;
    if (s.rangeHi[pp] - s.rangeLo[pp] + 1u <= s.leafMax)
      return;
  }
  unsigned pre = 0, escBuild = VR_END;
  bool escFound = false;
  while (haveParent) {
    const unsigned pp = pw & 0x7FFFFFFFu;
    const bool amRight = (pw & 0x80000000u) != 0u;
    const bool rightFirst = (s.subSize[pp] & 0x80000000u) != 0u;
    pre += 1u;
    if (amRight != rightFirst) { // second child: the first child's subtree comes before
      pre += sub_size(s, rightFirst ? s.childR[pp] : s.childL[pp]);
    } else if (!escFound) {      // first child: the walk continues with the sibling
      escBuild = node_of_child(s, rightFirst ? s.childL[pp] : s.childR[pp]);
      escFound = true;
    }
    if (pp == 0)
      break;
    pw = s.parentInt[pp];
  }
  const unsigned total = s.subSize[0] & 0x7FFFFFFFu;
  unsigned linkPre, linkBuild, mySize;
  const float *b;
  if (internal) {
    const unsigned lo = s.rangeLo[t], cnt = s.rangeHi[t] - lo + 1u;
    const unsigned w = s.subSize[t];
    mySize = w & 0x7FFFFFFFu;
    if (cnt <= s.leafMax) {
      linkPre = linkBuild = VR_LEAF | (cnt << 27) | lo;
    } else {
      linkPre = pre + 1u;
      linkBuild = node_of_child(s, (w & 0x80000000u) ? s.childR[t] : s.childL[t]);
    }
    b = s.nodeBox + 6 * (size_t)t;
  } else {
    mySize = 1u;
    linkPre = linkBuild = VR_LEAF | (1u << 27) | q;
    b = s.sbox + 6 * (size_t)q;
  }
  const unsigned escPre = pre + mySize >= total ? VR_END : pre + mySize;
  nodes[2 * (size_t)t] = make_float4(b[0], b[1], b[2], __uint_as_float(linkBuild));
  nodes[2 * (size_t)t + 1] = make_float4(b[3], b[4], b[5], __uint_as_float(escBuild));
  nodesPre[2 * (size_t)pre] = make_float4(b[0], b[1], b[2], __uint_as_float(linkPre));
  nodesPre[2 * (size_t)pre + 1] = make_float4(b[3], b[4], b[5], __uint_as_float(escPre));
}

// 16-byte form of the same nodes for the per-lane traversal: the box on a 16-bit grid of
// the scene (rounded outwards and widened by one cell, so the test stays conservative
// under the float rounding of the quantised-space slab test) + ONE link word:
//   internal: escape index (VR_QEND when none)        [first child = this + 1]
//   leaf    : VR_LEAF | cnt << 27 | first primitive   [escape      = this + 1]
__global__ void quantize_nodes_kernel(const float4 *nodes, unsigned numNodes, float bx, float by, float bz, float sx,
                                      float sy, float sz, uint4 *qnodes) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= numNodes)
    return;
  const float4 a = nodes[2 * (size_t)i], b = nodes[2 * (size_t)i + 1];
  const float base[3] = {bx, by, bz}, sc[3] = {sx, sy, sz};
  const float lo[3] = {a.x, a.y, a.z}, hi[3] = {b.x, b.y, b.z};
  unsigned ql[3], qh[3];
  for (int k = 0; k < 3; ++k) {
    const float l = floorf((lo[k] - base[k]) * sc[k]) - 1.f;
    const float h = ceilf((hi[k] - base[k]) * sc[k]) + 1.f;
    ql[k] = (unsigned)fminf(fmaxf(l, 0.f), 65535.f);
    qh[k] = (unsigned)fminf(fmaxf(h, 0.f), 65535.f);
  }
  const unsigned link = __float_as_uint(a.w), esc = __float_as_uint(b.w);
  const unsigned w = (link & VR_LEAF) ? link : (esc == VR_END ? VR_QEND : esc);
  qnodes[i] = make_uint4(ql[0] | (ql[1] << 16), ql[2] | (qh[0] << 16), qh[1] | (qh[2] << 16), w);
}

// PAIR nodes for the ordered per-lane walk (vr_device.hpp: pair_walk_lanes): entry i (i = pre-order index of
// an internal node) holds BOTH children — {box(c0), link(c0)} {box(c1), link(c1)}, 32 bytes in one cache
// line — so one visit decides both, descends into the nearer one and defers the other.
//   link: leaf -> its leaf word (VR_LEAF | cnt << 27 | first), internal -> its pre-order index
// c0 = i + 1, c1 = the node after c0's subtree.  A scene that is one leaf gets the pair {that leaf, nothing}.
__global__ void pair_nodes_kernel(const uint4 *qnodes, unsigned numNodes, uint4 *pnodes) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= numNodes)
    return;
  const uint4 me = qnodes[i];
  if (me.w & VR_LEAF) {
    if (i == 0u) { // the whole scene is one leaf
      pnodes[0] = me;
      pnodes[1] = make_uint4(0xFFFFFFFFu, 0x0000FFFFu, 0u, VR_LEAF); // lo = 65535 > hi = 0: never hit; empty leaf
    }
    return;
  }
  const unsigned c0 = i + 1u;
  const uint4 a = qnodes[c0];
  const unsigned c1 = (a.w & VR_LEAF) ? c0 + 1u : a.w;
  const uint4 b = qnodes[c1];
  pnodes[2 * (size_t)i] = make_uint4(a.x, a.y, a.z, (a.w & VR_LEAF) ? a.w : c0);
  pnodes[2 * (size_t)i + 1] = make_uint4(b.x, b.y, b.z, (b.w & VR_LEAF) ? b.w : c1);
}

// sorted boxes, leafOfOrig, primitive records in leaf order
__global__ void pack_kernel(SetupParams s) {
  const unsigned q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= s.n)
    return;
  const unsigned o = s.valsA[q];
  s.leafOfOrig[o] = q;
  s.order[q] = o;
  for (int k = 0; k < 6; ++k)
    s.sbox[6 * (size_t)q + k] = s.box[6 * (size_t)o + k];
  float4 *pr = reinterpret_cast<float4 *>(s.prims);
  if (s.geo == 0) {
    pr[2 * (size_t)q] = reinterpret_cast<const float4 *>(s.disk4)[o];
    pr[2 * (size_t)q + 1] = make_float4(s.normal3[3 * (size_t)o], s.normal3[3 * (size_t)o + 1],
                                        s.normal3[3 * (size_t)o + 2], __uint_as_float(o));
  } else {
    const float *a = s.verts + 3 * (size_t)s.tris[3 * (size_t)o];
    const float *b = s.verts + 3 * (size_t)s.tris[3 * (size_t)o + 1];
    const float *c = s.verts + 3 * (size_t)s.tris[3 * (size_t)o + 2];
    const float e1[3] = {a[0] - b[0], a[1] - b[1], a[2] - b[2]};
    const float e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    // Ng = cross(e2, e1), separate multiplies and subtract (no contraction)
    const float Ng[3] = {e2[1] * e1[2] - e2[2] * e1[1], e2[2] * e1[0] - e2[0] * e1[2], e2[0] * e1[1] - e2[1] * e1[0]};
    const float *nn = s.normal3 + 3 * (size_t)o;
    pr[4 * (size_t)q] = make_float4(a[0], a[1], a[2], __uint_as_float(o));
    pr[4 * (size_t)q + 1] = make_float4(e1[0], e1[1], e1[2], nn[0]);
    pr[4 * (size_t)q + 2] = make_float4(e2[0], e2[1], e2[2], nn[1]);
    pr[4 * (size_t)q + 3] = make_float4(Ng[0], Ng[1], Ng[2], nn[2]);
  }
}

// ---------------------------------------------------------------------------
// neighbourhood by BVH range query (disks).  Pass 0 counts, pass 1 fills.
// The caller's points (not the float4 disc buffer) define the distance test,
// like the reference (rayGeometryDisk.hpp:191: `init<Dim>(points, ...)`).
// ---------------------------------------------------------------------------
template <int PASS> __global__ void nb_kernel(SetupParams s) {
  const unsigned q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= s.n)
    return;
  const float4 *nodes = reinterpret_cast<const float4 *>(s.nodes);
  const unsigned me = s.order[q];
  const float px = s.points3[3 * (size_t)me], py = s.points3[3 * (size_t)me + 1], pz = s.points3[3 * (size_t)me + 2];
  const float dist = s.nbDist, dist2 = dist * dist;
  // query box: every disc whose centre is within `dist` has that centre inside it,
  // and a disc's box contains its centre
  const float qlo[3] = {px - dist, py - dist, s.D == 2 ? -FLT_MAX : pz - dist};
  const float qhi[3] = {px + dist, py + dist, s.D == 2 ? FLT_MAX : pz + dist};
  unsigned count = 0;
  const unsigned base = PASS == 1 ? s.nbOff[q] : 0u;
  unsigned node = 0;
  while (node != VR_END) {
    const float4 a = nodes[2 * (size_t)node], b = nodes[2 * (size_t)node + 1];
    const unsigned link = __float_as_uint(a.w), esc = __float_as_uint(b.w);
    const bool hit = a.x <= qhi[0] && b.x >= qlo[0] && a.y <= qhi[1] && b.y >= qlo[1] && a.z <= qhi[2] && b.z >= qlo[2];
    if (hit) {
      if (link & VR_LEAF) {
        const unsigned first = link & VR_LEAF_FIRST_MASK, cnt = (link >> 27) & 15u;
        for (unsigned k = 0; k < cnt; ++k) {
          const unsigned r = first + k;
          if (r == q)
            continue;
          const unsigned o = s.order[r];
          const float dx = px - s.points3[3 * (size_t)o], dy = py - s.points3[3 * (size_t)o + 1],
                      dz = pz - s.points3[3 * (size_t)o + 2];
          bool near = fabsf(dx) <= dist && fabsf(dy) <= dist && (s.D == 2 || fabsf(dz) <= dist);
          near = near && ((dx * dx + dy * dy) + dz * dz) <= dist2;
          if (near) {
            if (PASS == 1)
              s.nbIds[base + count] = r;
            else if (PASS == 2 && count < VR_NB_KEEP)
              s.nbTmp[(size_t)q * VR_NB_KEEP + count] = r;
            ++count;
          }
        }
        node = esc;
      } else {
        node = link;
      }
    } else {
      node = esc;
    }
  }
  if (PASS != 1)
    s.nbOff[q] = count;
  if (PASS == 2 && count > VR_NB_KEEP)
    s.nbTmp[(size_t)s.n * VR_NB_KEEP] = 1u; // (more neighbours than kept: the caller falls back to count + fill)
}

// pass 2's lists, packed behind the scanned offsets (the query itself — a range walk of the BVH per primitive, the most
// expensive kernel of a scene build — runs once instead of twice)
__global__ void nb_compact_kernel(SetupParams s) {
  const unsigned q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= s.n)
    return;
  const unsigned b = s.nbOff[q], e = s.nbOff[q + 1];
  for (unsigned j = b; j < e; ++j)
    s.nbIds[j] = s.nbTmp[(size_t)q * VR_NB_KEEP + (j - b)];
}

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
hipError_t launch_setup_bvh(const SetupParams &sp, unsigned *scanTmp, hipStream_t st) {
  SetupParams s = sp;
  const unsigned n = s.n;
  if (n == 0)
    return hipSuccess;
  const unsigned g256 = (n + 255) / 256;
  // bounds init: min = ord(+inf side), max = ord(-inf side)
  const unsigned initB[6] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u};
  hipError_t e = hipMemcpyAsync(s.bounds, initB, sizeof(initB), hipMemcpyHostToDevice, st);
  if (e != hipSuccess)
    return e;
  hipLaunchKernelGGL(prim_box_kernel, dim3(g256), dim3(256), 0, st, s);
  hipLaunchKernelGGL(morton_kernel, dim3(g256), dim3(256), 0, st, s);
  // radix sort (keysA, valsA) -> ping-pong with (keysB, valsB), 8 passes end in A
  const unsigned tiles = (n + SORT_TILE - 1) / SORT_TILE;
  u64 *kin = s.keysA, *kout = s.keysB;
  unsigned *vin = s.valsA, *vout = s.valsB;
  for (unsigned pass = 0; pass < 8; ++pass) {
    hipLaunchKernelGGL(sort_count_kernel, dim3(tiles), dim3(64), 0, st, kin, n, pass * 8, tiles, s.sortTable);
    e = launch_scan(s.sortTable, 256u * tiles, scanTmp, st);
    if (e != hipSuccess)
      return e;
    hipLaunchKernelGGL(sort_scatter_kernel, dim3(tiles), dim3(64), 0, st, kin, vin, kout, vout, n, pass * 8, tiles,
                       s.sortTable);
    u64 *tk = kin;
    kin = kout;
    kout = tk;
    unsigned *tv = vin;
    vin = vout;
    vout = tv;
  }
  // (8 passes: result is back in A)
  hipLaunchKernelGGL(pack_kernel, dim3(g256), dim3(256), 0, st, s);
  if (n > 1)
    hipLaunchKernelGGL(karras_kernel, dim3((n - 1 + 255) / 256), dim3(256), 0, st, s);
  return launch_fit_bvh(s, st);
}

// bottom-up fit + traversal-node emission over the resident radix tree (also the re-run with
// s.strictFence after a failed launch_bvh_check)
hipError_t launch_fit_bvh(const SetupParams &s, hipStream_t st) {
  const unsigned n = s.n;
  if (n == 0)
    return hipSuccess;
  if (n > 1) {
    hipError_t e = hipMemsetAsync(s.arrive, 0, (size_t)(n - 1) * 4, st);
    if (e != hipSuccess)
      return e;
    hipLaunchKernelGGL(fit_kernel, dim3((n + 255) / 256), dim3(256), 0, st, s);
  }
  hipLaunchKernelGGL(finalize_kernel, dim3((2 * n - 1 + 255) / 256), dim3(256), 0, st, s);
  return hipGetLastError();
}

// validation of the bottom-up fit (the hand-over in fit_kernel is the one place where the
// build relies on cross-workgroup ordering): every internal node's box must be exactly the
// union of its children's, its emitted size consistent.  Counts violations.
__global__ void bvh_check_kernel(SetupParams s, unsigned *bad) {
  const unsigned p = blockIdx.x * blockDim.x + threadIdx.x;
  if (s.n < 2 || p >= s.n - 1)
    return;
  const unsigned L = s.childL[p], R = s.childR[p];
  const float *a = (L & CHILD_LEAF) ? s.sbox + 6 * (size_t)(L & ~CHILD_LEAF) : s.nodeBox + 6 * (size_t)L;
  const float *b = (R & CHILD_LEAF) ? s.sbox + 6 * (size_t)(R & ~CHILD_LEAF) : s.nodeBox + 6 * (size_t)R;
  const float *o = s.nodeBox + 6 * (size_t)p;
  bool ok = true;
  for (int k = 0; k < 3; ++k)
    ok = ok && o[k] == fminf(a[k], b[k]) && o[3 + k] == fmaxf(a[3 + k], b[3 + k]);
  const unsigned sl = (L & CHILD_LEAF) ? 1u : (s.subSize[L] & 0x7FFFFFFFu);
  const unsigned sr = (R & CHILD_LEAF) ? 1u : (s.subSize[R] & 0x7FFFFFFFu);
  const unsigned cnt = s.rangeHi[p] - s.rangeLo[p] + 1u;
  ok = ok && (s.subSize[p] & 0x7FFFFFFFu) == (cnt <= s.leafMax ? 1u : 1u + sl + sr);
  if (!ok)
    atomicAdd(bad, 1u);
}

hipError_t launch_bvh_check(const SetupParams &s, unsigned *bad, hipStream_t st) {
  if (s.n < 2)
    return hipSuccess;
  hipLaunchKernelGGL(bvh_check_kernel, dim3((s.n - 1 + 255) / 256), dim3(256), 0, st, s, bad);
  return hipGetLastError();
}

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

// ---------------------------------------------------------------------------
// 64-ary box tree over the Morton-sorted primitives (packet query): a lowest-level node = union of
// the padded boxes of 64 consecutive primitives, a node of level l+1 = union of 64 consecutive nodes of level l.
// Implicit topology (children are contiguous), so there is nothing to sort or link; the
// Morton order makes 64 consecutive primitives a compact patch.  Stored top level first.
// ---------------------------------------------------------------------------
// lowest level: a node = 64 consecutive primitives (children implicit: leaf positions first .. first+cnt-1)
__global__ void wide_leafnodes_kernel(const float *sbox, unsigned n, float4 *wide, unsigned nodeBase,
                                      unsigned nodeCount) {
  const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= nodeCount)
    return;
  const unsigned first = 64u * g;
  const unsigned cnt = min(64u, n - first);
  float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  for (unsigned k = 0; k < cnt; ++k) {
    const float *b = sbox + 6 * (size_t)(first + k);
    for (int c = 0; c < 3; ++c) {
      lo[c] = fminf(lo[c], b[c]);
      hi[c] = fmaxf(hi[c], b[3 + c]);
    }
  }
  wide[2 * (size_t)(nodeBase + g)] = make_float4(lo[0], lo[1], lo[2], __uint_as_float(first));
  wide[2 * (size_t)(nodeBase + g) + 1] = make_float4(hi[0], hi[1], hi[2], __uint_as_float(cnt | VR_WIDE_PRIMS));
}

__global__ void wide_level_kernel(float4 *wide, unsigned childBase, unsigned childCount, unsigned nodeBase,
                                  unsigned nodeCount) {
  const unsigned g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= nodeCount)
    return;
  const unsigned first = childBase + 64u * g;
  const unsigned cnt = min(64u, childCount - 64u * g);
  float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  for (unsigned k = 0; k < cnt; ++k) {
    const float4 a = wide[2 * (size_t)(first + k)], b = wide[2 * (size_t)(first + k) + 1];
    lo[0] = fminf(lo[0], a.x);
    lo[1] = fminf(lo[1], a.y);
    lo[2] = fminf(lo[2], a.z);
    hi[0] = fmaxf(hi[0], b.x);
    hi[1] = fmaxf(hi[1], b.y);
    hi[2] = fmaxf(hi[2], b.z);
  }
  wide[2 * (size_t)(nodeBase + g)] = make_float4(lo[0], lo[1], lo[2], __uint_as_float(first));
  wide[2 * (size_t)(nodeBase + g) + 1] = make_float4(hi[0], hi[1], hi[2], __uint_as_float(cnt));
}

// entries the tree of n primitives needs (levels above the primitives)
size_t wide_tree_entries(unsigned n) {
  size_t total = 0, c = n;
  do {
    c = (c + 63) / 64;
    total += c;
  } while (c > 64);
  return total + 1;
}

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
    for (int k = 0; k < 3; ++k) { // the disc's own extent along axis k (as the BVH's boxes: vr_setup.hip, box_kernel)
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

// builds the tree from s.sbox (sorted, padded boxes); out3 = the root's {first child entry,
// child count | VR_WIDE_PRIMS if the root's children are the primitives themselves, 0}
hipError_t launch_wide_tree(const SetupParams &s, unsigned *out3, hipStream_t st) {
  const unsigned n = s.n;
  out3[0] = out3[1] = out3[2] = 0;
  if (n == 0)
    return hipSuccess;
  if (n <= 64) { // the root's children are the primitives
    out3[1] = n | VR_WIDE_PRIMS;
    return hipSuccess;
  }
  unsigned counts[8], nl = 0;
  counts[nl++] = (n + 63) / 64;
  while (counts[nl - 1] > 64) {
    counts[nl] = (counts[nl - 1] + 63) / 64;
    ++nl;
  }
  // memory order: top level first
  unsigned base[8];
  unsigned off = 0;
  for (int l = (int)nl - 1; l >= 0; --l) {
    base[l] = off;
    off += counts[l];
  }
  float4 *wide = reinterpret_cast<float4 *>(s.wide);
  hipLaunchKernelGGL(wide_leafnodes_kernel, dim3((counts[0] + 63) / 64), dim3(64), 0, st, s.sbox, n, wide, base[0],
                     counts[0]);
  for (unsigned l = 1; l < nl; ++l)
    hipLaunchKernelGGL(wide_level_kernel, dim3((counts[l] + 63) / 64), dim3(64), 0, st, wide, base[l - 1], counts[l - 1],
                       base[l], counts[l]);
  out3[0] = base[nl - 1];
  out3[1] = counts[nl - 1];
  return hipGetLastError();
}

hipError_t launch_quantize_nodes(const float *nodes, unsigned numNodes, const float *base3, const float *scale3,
                                 uint32_t *qnodes, uint32_t *pnodes, hipStream_t st) {
  if (numNodes == 0)
    return hipSuccess;
  hipLaunchKernelGGL(quantize_nodes_kernel, dim3((numNodes + 255) / 256), dim3(256), 0, st,
                     reinterpret_cast<const float4 *>(nodes), numNodes, base3[0], base3[1], base3[2], scale3[0],
                     scale3[1], scale3[2], reinterpret_cast<uint4 *>(qnodes));
  hipLaunchKernelGGL(pair_nodes_kernel, dim3((numNodes + 255) / 256), dim3(256), 0, st,
                     reinterpret_cast<const uint4 *>(qnodes), numNodes, reinterpret_cast<uint4 *>(pnodes));
  return hipGetLastError();
}

hipError_t launch_setup_neighbors(const SetupParams &s, int pass, hipStream_t st) {
  const unsigned g = (s.n + 255) / 256;
  if (s.n == 0)
    return hipSuccess;
  if (pass == 0)
    hipLaunchKernelGGL((nb_kernel<0>), dim3(g), dim3(256), 0, st, s);
  else if (pass == 1)
    hipLaunchKernelGGL((nb_kernel<1>), dim3(g), dim3(256), 0, st, s);
  else if (pass == 2) // count and keep (s.nbTmp; its overflow word zeroed by the caller)
    hipLaunchKernelGGL((nb_kernel<2>), dim3(g), dim3(256), 0, st, s);
  else                // pack pass 2's lists behind the scanned offsets
    hipLaunchKernelGGL(nb_compact_kernel, dim3(g), dim3(256), 0, st, s);
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
