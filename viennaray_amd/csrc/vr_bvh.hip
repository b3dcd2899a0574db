// vr_bvh.hip — device-side scene build: LBVH, 64-ary box tree and disk-neighbourhood CSR.
//
// The reference builds its acceleration structure inside the timed region
// (rtcJoinCommitScene, rayTraceKernel.hpp:91) and its point
// neighbourhood at setGeometry (rayGeometryDisk.hpp:191-192, recursive host
// vectors).  Here both are HIP kernels:
//
//   prim_box_kernel     primitive AABBs (oriented-disc extents r*sqrt(1-n_k^2),
//                       triangle min/max) + scene bounds (ordered-int atomics)
//   morton_kernel       63-bit Morton code of each box centre
//   radix sort          (vr_sort.hip: launch_sort_pairs) LSD, 8-bit digits, one wavefront per 1024-key tile,
//                       ballot-based stable ranking (no LDS scatter buffers)
//   karras_kernel       binary radix tree over the sorted codes (Karras 2012)
//   fit_kernel          bottom-up AABB fit with arrival counters; emits the subtree sizes and the
//                       source-side-first child order
//   finalize_kernel     traversal nodes {lo,link}{hi,escape} in pre-order: ranges of
//                       <= leafMax primitives collapse into leaves
//   pack_kernel         primitive records in leaf order
//   bvh_check_kernel    every internal box is the union of its children's, every emitted size consistent
//   quantize_nodes      16-byte nodes (16-bit conservative boxes) for per-lane traversal, pair_nodes on top
//   wide_*_kernel       64-ary box tree over the sorted primitives for the packet query
//   nb_kernel<PASS>     neighbourhood = stackless BVH range query around every
//                       disc centre (per-axis |d| <= dist and |d|^2 <= dist^2,
//                       rayPointNeighborhood.hpp:287-298), written as CSR of leaf
//                       positions
#include <hip/hip_runtime.h>

#include <cfloat>

#include "vr_kernels.hpp"
#include "vr_setup_common.hpp"
#include "vr_types.hpp"

namespace vr {

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
  e = launch_sort_pairs(s.keysA, s.valsA, s.keysB, s.valsB, n, s.sortTable, scanTmp, st);
  if (e != hipSuccess)
    return e;
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

// PAIR nodes for the ordered per-lane walk (vr_walk.hpp: pair_walk_lanes): entry i (i = pre-order index of
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

} // namespace vr
