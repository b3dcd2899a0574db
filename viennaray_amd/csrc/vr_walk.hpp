// vr_walk.hpp — the three BVH walks: per lane by escape links, per lane ordered (pair nodes), wave-uniform (gfx950).
#pragma once
#include "vr_diag_macros.hpp"
#include "vr_intersect.hpp"
namespace vr {

__device__ __forceinline__ V3 safe_inverse(const V3 &d) {
  const float dx = fabsf(d.x) < 1e-30f ? copysignf(1e-30f, d.x) : d.x;
  const float dy = fabsf(d.y) < 1e-30f ? copysignf(1e-30f, d.y) : d.y;
  const float dz = fabsf(d.z) < 1e-30f ? copysignf(1e-30f, d.z) : d.z;
  return V3{1.0f / dx, 1.0f / dy, 1.0f / dz};
}

// The per-lane walks' slab test rounds its bounds at the magnitude of o * inv, i.e. by a few ulp of the DISTANCE to the
// box (seven roundings: < 1.3e-6 of it once the origin is two scene extents away).  The boxes' own padding (4e-6 of the
// scene's scale, in space) covers that only while the origin lies within a few extents of the scene, and nothing covered
// the comparison with the closest hit so far: from far away, a box whose primitive TIES with that hit (two disks of one
// plane, the lower original id in the box visited second) was culled when its entry bound came out an ulp above h.t.
// The entry bound is therefore taken this much short before it is compared with the exit bound and with h.t.
constexpr float VR_SLAB_SLACK = 1.0f - 4e-6f;

// geometry, per-lane, escape links: every lane walks its own path over the pre-order nodes.  Kept for the
// absorbing flat-scene kernel (MODE 1), whose rounds are packets and which wants the single register of walk
// state, as the reference walk of the -DVR_SELFCHECK build and of vr_debug_intersect (VR_DEBUG_WALK=0); the
// kernels that walk a lot use pair_walk_lanes below.  Divergent lanes
// make every node fetch 64 separate requests, so this walk reads the 16-byte nodes:
// one dwordx4 per visit.  The slab test runs in the quantised frame (ray transformed
// once per call; per-axis scaling leaves t unchanged); boxes were rounded outwards
// by more than the rounding of this test, and a box only ever culls.
// `node` is the lane's cursor (resumable): the loop runs while at least `minLanes`
// lanes of the wave are still walking, then returns with the stragglers' cursors and
// closest hits intact.
template <int GEO>
__device__ __forceinline__ void bvh_walk_lanes(const TraceParams &p, bool part, const V3 &o, const V3 &d, float tnear,
                                               HitRec &h, unsigned &node, unsigned minLanes VR_DIAG_ARGS) {
  const uint4 *__restrict__ qnodes = reinterpret_cast<const uint4 *>(p.qnodes);
  const float4 *__restrict__ prims = reinterpret_cast<const float4 *>(p.prims);
  const V3 inv = safe_inverse(V3{d.x * p.qscale[0], d.y * p.qscale[1], d.z * p.qscale[2]});
  const V3 oi = V3{(o.x - p.qbase[0]) * p.qscale[0] * inv.x, (o.y - p.qbase[1]) * p.qscale[1] * inv.y,
                   (o.z - p.qbase[2]) * p.qscale[2] * inv.z};
  if (!part)
    node = VR_END;
  const float invDD = 1.0f / vdot(d, d);
  // Two alternating phases ("while-while"): a lane SEARCHES for leaves whose box it hits.
  // The first such leaf is only remembered (`pend`) and the lane searches on
  // (speculatively: it may visit nodes the pending leaf's hit would have culled); at a
  // second leaf it parks on that node.  When a given share of the lanes under way are
  // parked, or nobody searches any more, the pending leaves' primitives are tested
  // together.  Testing a leaf the moment one lane reaches it would run the (long)
  // primitive test with a handful of lanes on almost every step.
  unsigned pend = 0u; // pending leaf link (VR_LEAF bit set) or 0
  // The loop bodies are PREDICATED, not branched: a lane that is not searching (parked, done, or
  // never took part) runs the step on node 0 and discards it.  An exec-masked step costs the same
  // issue slots as a full one, and the mask juggling of a divergent `if` was a third of the
  // instructions of this loop; two steps run between the wave-level votes for the same reason.
  for (;;) {
    bool parked = false;
    for (;;) {
      const bool search0 = node < p.numNodes && !parked;
      const unsigned long long sm = ballot64(search0);
      if (!sm)
        break;
      const unsigned long long km = ballot64(parked);
      if (100u * (unsigned)__popcll(km) >= p.walkPark * (unsigned)__popcll(km | sm))
        break;
#pragma unroll
      for (int rep = 0; rep < 2; ++rep) {
        const bool search = node < p.numNodes && !parked;
#ifdef VR_DIAG
        if (search) {
          DIAG(1);
        }
#endif
        const uint4 nd = qnodes[search ? node : 0u];
        const float lx = (float)(nd.x & 0xFFFFu), ly = (float)(nd.x >> 16), lz = (float)(nd.y & 0xFFFFu);
        const float hx = (float)(nd.y >> 16), hy = (float)(nd.z & 0xFFFFu), hz = (float)(nd.z >> 16);
        const float tx0 = __builtin_fmaf(lx, inv.x, -oi.x), tx1 = __builtin_fmaf(hx, inv.x, -oi.x);
        const float ty0 = __builtin_fmaf(ly, inv.y, -oi.y), ty1 = __builtin_fmaf(hy, inv.y, -oi.y);
        const float tz0 = __builtin_fmaf(lz, inv.z, -oi.z), tz1 = __builtin_fmaf(hz, inv.z, -oi.z);
        const float tEntry = fmaxf(fmaxf(fminf(tx0, tx1), fminf(ty0, ty1)), fmaxf(fminf(tz0, tz1), tnear)) * VR_SLAB_SLACK;
        const float tExit = fminf(fminf(fmaxf(tx0, tx1), fmaxf(ty0, ty1)), fmaxf(tz0, tz1));
        const unsigned link = nd.w;
        const bool leaf = (link & VR_LEAF) != 0u;
        const bool hitBox = tEntry <= tExit && tEntry <= h.t;
        const bool take = search && hitBox && leaf;
        const bool park = take && pend != 0u; // second leaf: wait here (the node is visited again afterwards)
        pend = (take && pend == 0u) ? link : pend;
        parked = parked || park;
        // pre-order: first child of an internal node / escape of a leaf = next node
        const unsigned nxt = (hitBox || leaf) ? node + 1u : link;
        node = (search && !park) ? nxt : node;
      }
    }
    if (ballot64(pend != 0u)) {
      const unsigned first = pend & VR_LEAF_FIRST_MASK;
      const unsigned cnt = pend ? (pend >> 27) & 15u : 0u;
      for (unsigned i = 0; ballot64(i < cnt); ++i) {
        const bool on = i < cnt;
#ifdef VR_DIAG
        if (on) {
          DIAG(2);
        }
#endif
        const unsigned q = on ? first + i : 0u;
        float t;
        if (GEO == 0) {
          const float4 c4 = prims[2 * q];
          if (on && disc_may_hit(o, d, invDD, c4)) { // (exec-masked: lanes that fail fetch nothing more)
            const float4 n4 = prims[2 * q + 1];
            const bool ok = hit_disc(o, d, tnear, c4, mk(n4.x, n4.y, n4.z), t);
            hit_update(h, ok, t, __float_as_uint(n4.w), q);
          }
        } else {
          const float4 a = prims[4 * q], b = prims[4 * q + 1], c = prims[4 * q + 2], e = prims[4 * q + 3];
          const bool ok =
              hit_tri(o, d, tnear, mk(a.x, a.y, a.z), mk(b.x, b.y, b.z), mk(c.x, c.y, c.z), mk(e.x, e.y, e.z), t);
          hit_update(h, on && ok, t, __float_as_uint(a.w), q);
        }
      }
      pend = 0u;
    }
    if ((unsigned)__popcll(ballot64(node < p.numNodes)) < minLanes)
      break;
  }
}

// ---------------------------------------------------------------------------
// geometry, per-lane, ORDERED: the walk of bounced rays.  bvh_walk_lanes follows the escape links of a
// pre-order layout: one node (one 16-byte gather, one dependent cache access) per box test, and the
// order of the children is fixed at build time (source side first) — right for primary rays, wrong for
// half of the bounced ones, which then cannot be culled by a close hit.  Here a visit reads a PAIR node
// (both children of an internal node, 32 bytes of one line), tests both boxes, descends into the NEARER
// child and defers the other on a per-lane stack whose first SD entries live in LDS ([entry][lane]: conflict
// free) and the (rare) rest in a per-wave global slab.  Half the dependent accesses per box test, and the
// near-first order finds the closest hit early, so far subtrees fail `tEntry <= h.t` when they are popped.
// The closest-hit rule makes the result independent of the order: bit-identical to bvh_walk_lanes.
//   `node`: cursor — 0 = fresh (root pair), VR_END = finished, else a pair index or a leaf word.
//   `sp`:   stack depth of the lane (the caller keeps it with `node` between rounds).
// ---------------------------------------------------------------------------
template <int SD>
__device__ __forceinline__ void walk_push(unsigned *stackS, unsigned *stackG, unsigned long long *errFlag, unsigned &sp,
                                          unsigned v) {
  if (sp < (unsigned)SD)
    stackS[sp * VR_BLOCK] = v;
  else if (sp < (unsigned)SD + VR_STACK_GLOBAL)
    stackG[(sp - (unsigned)SD) * 64u] = v;
  else
    *errFlag = 1ull; // deeper than any tree the builder emits: reported by vr_apply_finish, never silent
  ++sp;
}
template <int SD> __device__ __forceinline__ unsigned walk_pop(const unsigned *stackS, const unsigned *stackG, unsigned &sp) {
  --sp;
  if (sp < (unsigned)SD)
    return stackS[sp * VR_BLOCK];
  return sp < (unsigned)SD + VR_STACK_GLOBAL ? stackG[(sp - (unsigned)SD) * 64u] : VR_END;
}

// stackS: this lane's column of the LDS stack (entry e at stackS[e * VR_BLOCK]); stackG: this lane's column of
// the wave's global slab (entry e at stackG[e * 64])
// pnodes / prims: the pair nodes and primitive records — global memory, or the LDS copies of MODE 4
// the pending leaves of a wave: every lane tests the primitives of ITS leaf word `pend` (0: none)
template <int GEO, bool LEAF2>
__device__ __forceinline__ void walk_leaf_tests(const float4 *__restrict__ prims, const V3 &o, const V3 &d, float invDD,
                                                float tnear, HitRec &h, unsigned &pend VR_DIAG_ARGS) {
    if (ballot64(pend != 0u)) {
      const unsigned first = pend & VR_LEAF_FIRST_MASK;
      const unsigned cnt = pend ? (pend >> 27) & 15u : 0u;
      for (unsigned i = 0; ballot64(i < cnt); i += ((GEO == 0 && LEAF2) ? 2u : 1u)) {
        const bool on = i < cnt;
#ifdef VR_DIAG
        if (on) {
          DIAG(2);
        }
#endif
        const unsigned q = on ? first + i : 0u;
        float t;
        if (GEO == 0) {
          // two disks per pass, all four record words requested together
          const bool on2 = LEAF2 && i + 1u < cnt;
          const unsigned q2 = on2 ? q + 1u : q;
          const float4 c4 = prims[2 * q];
          const float4 n4 = prims[2 * q + 1];
          const float4 c5 = prims[2 * q2];
          const float4 n5 = prims[2 * q2 + 1];
          asm volatile("" ::"v"(c4.x), "v"(n4.x), "v"(c5.x), "v"(n5.x));
          if (on && disc_may_hit(o, d, invDD, c4)) {
            const bool ok = hit_disc(o, d, tnear, c4, mk(n4.x, n4.y, n4.z), t);
            hit_update(h, ok, t, __float_as_uint(n4.w), q);
          }
          if (on2 && disc_may_hit(o, d, invDD, c5)) {
            const bool ok = hit_disc(o, d, tnear, c5, mk(n5.x, n5.y, n5.z), t);
            hit_update(h, ok, t, __float_as_uint(n5.w), q2);
          }
        } else {
          const float4 a = prims[4 * q], b = prims[4 * q + 1], c = prims[4 * q + 2], e = prims[4 * q + 3];
          const bool ok =
              hit_tri(o, d, tnear, mk(a.x, a.y, a.z), mk(b.x, b.y, b.z), mk(c.x, c.y, c.z), mk(e.x, e.y, e.z), t);
          hit_update(h, on && ok, t, __float_as_uint(a.w), q);
        }
      }
      pend = 0u;
    }
}

// LEAF2: the leaf test takes two disks per pass, all four record words in flight together (8 more live registers:
// not for the 72-VGPR absorbing kernel)
template <int GEO, int SD, bool LEAF2 = true>
__device__ __forceinline__ void pair_walk_lanes(const TraceParams &p, const uint4 *__restrict__ pnodes,
                                                const float4 *__restrict__ prims, unsigned *stackS, unsigned *stackG,
                                                bool part, const V3 &o, const V3 &d, float tnear, HitRec &h,
                                                unsigned &node, unsigned &sp, unsigned minLanes VR_DIAG_ARGS) {
  const V3 inv = safe_inverse(V3{d.x * p.qscale[0], d.y * p.qscale[1], d.z * p.qscale[2]});
  const V3 oi = V3{(o.x - p.qbase[0]) * p.qscale[0] * inv.x, (o.y - p.qbase[1]) * p.qscale[1] * inv.y,
                   (o.z - p.qbase[2]) * p.qscale[2] * inv.z};
  if (!part)
    node = VR_END;
  sp = node == 0u ? 0u : sp;
  const float invDD = 1.0f / vdot(d, d);
  unsigned long long *const errFlag = p.counters + C_WALK_OVERFLOW;
  unsigned pend = 0u; // pending leaf word or 0
  for (;;) {
    bool parked = false; // at a second leaf while the first is still pending
    for (;;) {
      const unsigned long long sm = ballot64(node != VR_END && !parked);
      if (!sm)
        break;
      const unsigned long long km = ballot64(parked);
      if (100u * (unsigned)__popcll(km) >= p.walkPark * (unsigned)__popcll(km | sm))
        break;
#pragma unroll
      for (int rep = 0; rep < 2; ++rep) {
        const bool live = node != VR_END && !parked;
        const bool atLeaf = live && (node & VR_LEAF) != 0u; // (a deferred child that is a leaf, popped)
        const bool visit = live && !atLeaf;
#ifdef VR_DIAG
        if (visit) {
          DIAG(1);
        }
        if (node != VR_END) { // (lanes whose walk is not finished: searching, at a leaf, or parked)
          DIAG(7);
        }
#endif
        const size_t idx = visit ? (size_t)node : 0u;
        const uint4 a = pnodes[2 * idx], b = pnodes[2 * idx + 1];
        bool hit0, hit1;
        float e0, e1;
        {
          const float lx = (float)(a.x & 0xFFFFu), ly = (float)(a.x >> 16), lz = (float)(a.y & 0xFFFFu);
          const float hx = (float)(a.y >> 16), hy = (float)(a.z & 0xFFFFu), hz = (float)(a.z >> 16);
          const float tx0 = __builtin_fmaf(lx, inv.x, -oi.x), tx1 = __builtin_fmaf(hx, inv.x, -oi.x);
          const float ty0 = __builtin_fmaf(ly, inv.y, -oi.y), ty1 = __builtin_fmaf(hy, inv.y, -oi.y);
          const float tz0 = __builtin_fmaf(lz, inv.z, -oi.z), tz1 = __builtin_fmaf(hz, inv.z, -oi.z);
          e0 = fmaxf(fmaxf(fminf(tx0, tx1), fminf(ty0, ty1)), fmaxf(fminf(tz0, tz1), tnear)) * VR_SLAB_SLACK;
          const float x0 = fminf(fminf(fmaxf(tx0, tx1), fmaxf(ty0, ty1)), fmaxf(tz0, tz1));
          hit0 = e0 <= x0 && e0 <= h.t;
        }
        {
          const float lx = (float)(b.x & 0xFFFFu), ly = (float)(b.x >> 16), lz = (float)(b.y & 0xFFFFu);
          const float hx = (float)(b.y >> 16), hy = (float)(b.z & 0xFFFFu), hz = (float)(b.z >> 16);
          const float tx0 = __builtin_fmaf(lx, inv.x, -oi.x), tx1 = __builtin_fmaf(hx, inv.x, -oi.x);
          const float ty0 = __builtin_fmaf(ly, inv.y, -oi.y), ty1 = __builtin_fmaf(hy, inv.y, -oi.y);
          const float tz0 = __builtin_fmaf(lz, inv.z, -oi.z), tz1 = __builtin_fmaf(hz, inv.z, -oi.z);
          e1 = fmaxf(fmaxf(fminf(tx0, tx1), fminf(ty0, ty1)), fmaxf(fminf(tz0, tz1), tnear)) * VR_SLAB_SLACK;
          const float x1 = fminf(fminf(fmaxf(tx0, tx1), fmaxf(ty0, ty1)), fmaxf(tz0, tz1));
          hit1 = e1 <= x1 && e1 <= h.t;
        }
        const bool both = hit0 && hit1, any = hit0 || hit1;
#ifdef VR_DIAG
        if (visit && !any) {
          DIAG(14);
        }
        if (visit && both) {
          DIAG(15);
        }
#endif
        const bool second = hit1 && (!hit0 || e1 < e0); // child 1 is the nearer one
        const unsigned nearL = second ? b.w : a.w, farL = second ? a.w : b.w;
        // a leaf goes into the pending slot when that is free; with the slot taken the lane parks on it
        const bool nearLeaf = (nearL & VR_LEAF) != 0u;
        const bool takeNear = visit && any && nearLeaf && pend == 0u;
        const bool takeSelf = atLeaf && pend == 0u;
        const bool park = atLeaf && pend != 0u;
        pend = takeNear ? nearL : (takeSelf ? node : pend);
        // where next: the nearer child, or — nothing (more) to enter here — the far child / the stack
        const bool descend = visit && any && !takeNear;
        const bool toFar = takeNear && both;
        const bool pop = (visit && !any) || (takeNear && !both) || takeSelf;
        if (descend && both)
          walk_push<SD>(stackS, stackG, errFlag, sp, farL);
        unsigned nxt = descend ? nearL : (toFar ? farL : node);
        if (pop)
          nxt = sp ? walk_pop<SD>(stackS, stackG, sp) : VR_END;
        node = nxt;
        parked = parked || park;
      }
    }
    TICK(2);
    walk_leaf_tests<GEO, LEAF2>(prims, o, d, invDD, tnear, h, pend VR_DIAG_PASS);
    TICK(3);
    if ((unsigned)__popcll(ballot64(node != VR_END)) < minLanes)
      break;
  }
}

// ---------------------------------------------------------------------------
// geometry, wave-uniform ("packet"): the 64 rays of a wavefront that were sorted
// into the same far-plane cell walk the UNION of their paths in lock step.  The
// node index is a scalar, node and primitive records come through the scalar
// cache (s_load, constant address space) instead of 64 per-lane vector loads,
// and there is no per-lane exec masking inside the traversal.  A lane that
// misses a box still runs the subtree's primitive tests; those are exact, so the
// selected hit is unchanged (the box test only ever culls).
typedef float vf4 __attribute__((ext_vector_type(4)));
typedef const vf4 __attribute__((address_space(4))) *ConstF4;

// `budget` bounds the number of node visits: a packet whose rays turn out to be
// incoherent (union of paths much larger than one path) gives up and returns false;
// the hits found so far are real hits and stay in `h`, the caller finishes with the
// per-lane traversal.  Besides the hard budget the walk keeps a running efficiency
// figure in scalar registers: `wants` = sum over visited nodes of the lanes whose own
// box test passed.  wants / lanes is the mean length of ONE ray's path; when the union
// walked so far exceeds `ratio` times that (plus a start-up allowance) the per-lane
// traversal is cheaper and the packet gives up (small scenes never reach the hard
// budget, so this is what protects them).
template <int GEO>
__device__ __forceinline__ bool bvh_hit_packet(const TraceParams &p, bool part, const V3 &o, const V3 &d, float tnear,
                                               HitRec &h, unsigned budget, unsigned ratio VR_DIAG_ARGS) {
  if (p.numPrims == 0)
    return true;
  const unsigned long long partMask = ballot64(part);
  const unsigned lanes = (unsigned)__popcll(partMask);
  unsigned wants = 16u * lanes; // start-up allowance: 16 visits
  unsigned visits = 0;
  ConstF4 nodes = (ConstF4)(p.nodes);
  ConstF4 prims = (ConstF4)(p.prims);
  const V3 inv = safe_inverse(d);
  const V3 oi = V3{o.x * inv.x, o.y * inv.y, o.z * inv.z};
  unsigned node = 0; // wave-uniform
  while (node != VR_END) {
    if (visits == budget || visits * lanes > ratio * wants)
      return false;
    ++visits;
    if (part) {
      DIAG(3);
    }
    const vf4 q0 = nodes[2 * node];
    const vf4 q1 = nodes[2 * node + 1];
    const float tx0 = __builtin_fmaf(q0.x, inv.x, -oi.x), tx1 = __builtin_fmaf(q1.x, inv.x, -oi.x);
    const float ty0 = __builtin_fmaf(q0.y, inv.y, -oi.y), ty1 = __builtin_fmaf(q1.y, inv.y, -oi.y);
    const float tz0 = __builtin_fmaf(q0.z, inv.z, -oi.z), tz1 = __builtin_fmaf(q1.z, inv.z, -oi.z);
    const float tEntry = fmaxf(fmaxf(fminf(tx0, tx1), fminf(ty0, ty1)), fmaxf(fminf(tz0, tz1), tnear));
    const float tExit = fminf(fminf(fmaxf(tx0, tx1), fmaxf(ty0, ty1)), fmaxf(tz0, tz1));
    const unsigned link = __builtin_amdgcn_readfirstlane(__float_as_uint(q0.w));
    const unsigned esc = __builtin_amdgcn_readfirstlane(__float_as_uint(q1.w));
    // (tEntry <= min(tExit, h.t), as two compares: a min with the loop-carried h.t costs a
    //  canonicalising v_max besides the v_min.
    //  Votes are taken per comparison and combined as scalar masks: a vote on a combined
    //  condition is lowered through a materialised 0/1 value, two more VALU per visit.)
    const unsigned long long want = partMask & ballot64(tEntry <= tExit) & ballot64(tEntry <= h.t);
    wants += (unsigned)__popcll(want);
    if (want) {
      if (link & VR_LEAF) {
        const unsigned first = link & VR_LEAF_FIRST_MASK;
        const unsigned cnt = (link >> 27) & 15u;
        for (unsigned i = 0; i < cnt; ++i) {
          if (part) {
            DIAG(4);
          }
          const unsigned q = first + i;
          float t;
          if (GEO == 0) {
            const vf4 c4v = prims[2 * q];
            const vf4 n4 = prims[2 * q + 1];
            const bool ok = hit_disc(o, d, tnear, make_float4(c4v.x, c4v.y, c4v.z, c4v.w), mk(n4.x, n4.y, n4.z), t);
            hit_update(h, part && ok, t, __float_as_uint(n4.w), q);
          } else {
            const vf4 a = prims[4 * q], b = prims[4 * q + 1], c = prims[4 * q + 2], e = prims[4 * q + 3];
            const bool ok =
                hit_tri(o, d, tnear, mk(a.x, a.y, a.z), mk(b.x, b.y, b.z), mk(c.x, c.y, c.z), mk(e.x, e.y, e.z), t);
            hit_update(h, part && ok, t, __float_as_uint(a.w), q);
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
  return true;
}

} // namespace vr
