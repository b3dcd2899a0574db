// vr_packet_query.hpp — the wave-uniform search by box (packet query) and the relief clip of its rays (gfx950).
#pragma once
#include "vr_planar_disks.hpp"
#include "vr_planar_lattice.hpp"
#include "vr_walk.hpp"
namespace vr {

// ---------------------------------------------------------------------------
// A ray's stretch through the LOCAL relief (ReliefParams, vr_types.hpp) instead of through the scene box.  The tiles of
// the relief field under the ray are walked from t0 to t1 (its stretch inside the scene box); inside a tile the ray can
// only meet a primitive while its height lies within the tile's [lo, hi] — every primitive that reaches into the tile
// lies in that range — so [tA, tB], the hull of those sub-stretches over all tiles walked, holds every point at which
// the ray meets ANY primitive (closest hit and neighbour crossings alike).  tA > tB: the ray meets nothing.
// Rounding: the walk may file a sliver of the ray under the neighbouring tile; the field's pad (1e-5 of the largest
// coordinate, three orders above the rounding of a position) makes that tile's range hold the primitive as well.
// After VR_RELIEF_STEPS tiles (a grazing ray that the generator did not file apart) the rest of the stretch is kept whole.
// ---------------------------------------------------------------------------
// Returns true for a lane whose walk was cut short after STEPS tiles (the rest of its stretch is then kept whole).
template <int STEPS = VR_RELIEF_STEPS>
__device__ __forceinline__ bool relief_clip(const float *__restrict__ wallS, bool on, const V3 &o, const V3 &d, float t0, float t1,
                                            float &tA, float &tB) {
  typedef float F2 __attribute__((ext_vector_type(2)));
  typedef const __attribute__((address_space(1))) F2 *GlobalF2;
  const GlobalF2 field = reinterpret_cast<GlobalF2>(((unsigned long long)__float_as_uint(wallS[VR_F_RF_PTR_HI]) << 32) |
                                                    __float_as_uint(wallS[VR_F_RF_PTR_LO]));
  const int ax = __float_as_int(wallS[VR_F_RAYDIR]), a1 = __float_as_int(wallS[VR_F_FIRSTDIR]), a2 = __float_as_int(wallS[VR_F_SECONDDIR]);
  const int nx = __float_as_int(wallS[VR_F_RF_NX]), ny = __float_as_int(wallS[VR_F_RF_NY]);
  const float T = wallS[VR_F_RF_TILE], invT = wallS[VR_F_RF_INVT], lo1 = wallS[VR_F_RF_LO1], lo2 = wallS[VR_F_RF_LO2];
  const float oz = getc(o, ax), dz = getc(d, ax), o1 = getc(o, a1), d1 = getc(d, a1);
  const float o2 = ny > 1 ? getc(o, a2) : 0.f, d2 = ny > 1 ? getc(d, a2) : 0.f;
  const float big = 3.0e38f;
  tA = big;
  tB = -big;
  int ix = (int)floorf((o1 + d1 * t0 - lo1) * invT), iy = ny > 1 ? (int)floorf((o2 + d2 * t0 - lo2) * invT) : 0;
  ix = ix < 0 ? 0 : (ix >= nx ? nx - 1 : ix);
  iy = iy < 0 ? 0 : (iy >= ny ? ny - 1 : iy);
  const int sx = d1 > 0.f ? 1 : -1, sy = d2 > 0.f ? 1 : -1;
  const float inv1 = d1 != 0.f ? 1.0f / d1 : 0.f, inv2 = d2 != 0.f ? 1.0f / d2 : 0.f;
  float tx = d1 != 0.f ? (lo1 + (float)(ix + (d1 > 0.f ? 1 : 0)) * T - o1) * inv1 : big;
  float ty = d2 != 0.f ? (lo2 + (float)(iy + (d2 > 0.f ? 1 : 0)) * T - o2) * inv2 : big;
  const float dtx = T * fabsf(inv1), dty = T * fabsf(inv2);
  const float invz = dz != 0.f ? 1.0f / dz : 0.f;
  // (Skipping the air above the relief first — down to the height field's 3 x 3-tile maximum, one look-up — was built and
  //  measured in round 4: +- 0 on a plane with a bump and on the rippled sheet, the walk being at most six tiles anyway;
  //  started BELOW a tile's top it also made the query's box too low for the follow-up segments.  Removed.)
  float tc = t0;
  bool go = on && t0 <= t1, cut = false;
  for (int s = 0; ballot64(go); ++s) {
    if (go) {
      const float tn = fminf(fminf(tx, ty), t1);
      // (staging the wave's window of tiles in LDS first — one load per lane, then LDS reads in the walk — was built and
      //  measured in round 4: +- 0, the tiles are L1 hits; the lists it used now hold the frontier cache)
      const F2 f = field[iy * nx + ix];
      const float z0 = oz + dz * tc, z1 = oz + dz * tn;
      if (fmaxf(z0, z1) >= f.x && fminf(z0, z1) <= f.y) {
        float ta = tc, tb = tn;
        if (dz != 0.f) {
          const float q0 = (f.x - oz) * invz, q1 = (f.y - oz) * invz;
          ta = fmaxf(ta, fminf(q0, q1));
          tb = fminf(tb, fmaxf(q0, q1));
        }
        tA = fminf(tA, ta);
        tB = fmaxf(tB, tb);
      }
      if (!(tn < t1)) {
        go = false;
      } else if (s == STEPS - 1) { // (too many tiles: the rest of the stretch as it is)
        tA = fminf(tA, tn);
        tB = t1;
        go = false;
        cut = true;
      } else {
        if (tx <= ty) {
          ix += sx;
          tx += dtx;
        } else {
          iy += sy;
          ty += dty;
        }
        go = (unsigned)ix < (unsigned)nx && (unsigned)iy < (unsigned)ny; // (beyond the field: beyond the scene box)
        tc = tn;
      }
    }
  }
  return cut;
}

// ---------------------------------------------------------------------------
// geometry, wave-uniform by BOX ("packet query"): for rays that are close together where it
// matters.  Every participating ray is clipped to the scene's box; the box Q around all those
// clipped segments (six wave-wide min/max reductions) contains every point at which any of the
// rays can meet a primitive.  The 64-ary box tree (TraceParams::wide) is then searched for Q
// breadth first with the LANES AS CHILDREN: one coalesced load and one box-box test per
// visited node for 64 children at once, 3-4 levels for 10^6 primitives — instead of ~50
// scalar node visits with a 64-ray slab test each.  The primitives whose own box meets Q
// are tested exactly against every ray (records through the scalar cache, as in
// bvh_hit_packet); the closest-hit rule makes the result independent of how candidates were
// found.  Pays when Q is small: sorted primary rays on any scene whose relief is small against
// its extent, and ALL segments of a flat scene (a bounced ray leaves the thin scene box at
// once, whatever its direction).  Gives up (false, nothing touched) when a level's frontier or
// the candidate list outgrows its limit; the caller then walks as before.
// ---------------------------------------------------------------------------

// What a completed packet query leaves behind for the crediting of disks (pq_credit, vr_trace.hip):
// candidate c's leaf position and centre are record c of a small per-wave LDS table (written by the
// lane that holds the candidate's record, read back by all lanes at once: one ds_write_b128 / one
// broadcast ds_read_b128 per candidate instead of four v_writelane / v_readlane sequences), and bit c of each lane's
// `local` says whether that lane's ray passes the neighbour test on candidate c
// (checkLocalIntersection, rayTraceKernel.hpp:462-507).  Every disk a ray can be credited to is
// among the candidates: the test only passes where the ray crosses the disk, the disk lies in the
// scene box, and Q covers every participating ray from its origin to where it leaves that box.

#ifndef VR_PQ_KEEP
#define VR_PQ_KEEP 12 // leaf nodes a packet query's frontier cache keeps per wave (<= 16: the compacted list starts at lst[16])
#endif
struct PqCands {
  VR_LDS U4 *rec; // this wave's candidate records in LDS: {leaf position, centre.xyz as bits}, VR_PQ_CANDS entries
  unsigned long long local;
  unsigned count; // wave-uniform
  bool box;       // KEEPQ: records VR_PQ_BOX, + 1 hold the query's box (false: no ray reached the scene, nothing stored)
  unsigned mine;  // per lane: the candidate that is this lane's closest hit so far (valid where the hit came from the query)
  PlanarRound round; // ROUND: the round's point and thresholds, the caller's (trace_kernel computes them before the walls)
  unsigned slots;    // pq_hit_lattice_lanes alone, per lane: the window slots of the lane's four corners, a byte each (VR_PQ_NO_SLOT: none)
};
constexpr unsigned VR_PQ_CANDS = 52; // >= 2 * pqMaxCand + 1 (pqMaxCand <= 24, vr_knobs.cpp) + the two records below
// KEEPQ: records 50 / 51 keep the query's (padded) box {lo.xyz, -}{hi.xyz, -} for the round's follow-up segments
// (trace_kernel, "follow-up segments"); PqCands::box says whether there is one (stored as an "empty box", two constant
// 16-byte tuples were hoisted out of the round loop, spilled, and reloaded from scratch in every round)
constexpr unsigned VR_PQ_BOX = 50;
// records VR_PQ_NRM + c: candidate c's {normal.xyz, radius} — with record c everything the state machine (normal of the
// closest disk), the crediting and the follow-up segments need of a candidate, read from LDS instead of from its
// primitive record in global memory
constexpr unsigned VR_PQ_NRM = 52;
constexpr unsigned VR_PQ_RECORDS = 2 * 52;

// lst: 128 dwords of LDS private to this wave
// FRAME_LDS: the scene box and the padding come from the LDS frame `wallS` (see hit_walls_lds)
// RELIEF: the rays are clipped to the local relief (relief_clip) instead of to the scene box
// CACHE (the flat-scene kernels): consecutive rounds of a wave are neighbours in space — its bins follow a boustrophedon
// path — and the descent of the 64-ary tree is latency: three dependent node loads before the first primitive record
// (27 % of the flat kernel's wave time, -DVR_DIAG sub-phase timers).  A query therefore searches with its box ENLARGED by
// pqMargin and leaves its last-level frontier (the leaf nodes meeting the enlarged box S: complete for every box inside
// S, at most 12) with S in the wave's LDS lists (lst[0..], lst[64..]: the entries; lst[32..37]: S; lst[38]: their number;
// lst[39]: valid; cboxes: the leaf nodes' own boxes); a later round whose box lies inside S filters the kept nodes by ITS
// box — from LDS, no node load — and goes straight to the primitive records of those that meet it: the very nodes an
// exact descent would have found.  The candidates are filtered with the round's own box as before: bit-identical.
// LEAN (the 3-D absorbing flat-scene kernels): the candidate loop's disc tests in their branch-free forms (hit_disc_lds)
// UNIFORM (LEAN, for a launch whose disks all have one normal and one radius — the frame's VR_F_UD_*): what those tests
// take from the ray and the normal alone is computed once per round, before the candidate loop (hit_disc_uniform)
// PLANAR (UNIFORM, for disks that also share a plane normal to a coordinate axis — the frame's VR_F_PD_*): the point where the
// ray crosses that plane is the ray's own; the two divisions, the two points and the range tests once per round, a
// distance to the centre per candidate (vr_planar_disks.hpp has the argument)
// ROUND (PLANAR): that point is computed once, by the caller (cd.round), and serves both candidate tests; the query's box is
// the box around the wave's points, four reductions and no division, in place of the box around the rays' stretches
// through the scene box (vr_planar_disks.hpp (1), (2))
template <int GEO, bool CREDIT, bool FRAME_LDS = false, bool KEEPQ = false, bool RELIEF = false, bool CACHE = false, bool LEAN = false,
          bool UNIFORM = false, bool PLANAR = false, bool ROUND = false>
__device__ __forceinline__ bool pq_hit_packet(const TraceParams &p, bool part, const V3 &o, const V3 &d, float tnear,
                                              HitRec &h, volatile VR_LDS unsigned *lst, PqCands &cd,
                                              const float *__restrict__ wallS, volatile VR_LDS float *cboxes, float tWall VR_DIAG_ARGS) {
  const unsigned lane = threadIdx.x & 63u;
  // the ray's stretch inside the scene box
  const V3 inv = safe_inverse(d);
  const float tx0 = ((FRAME_LDS ? wallS[VR_F_SCENE_LO] : p.sceneLo[0]) - o.x) * inv.x, tx1 = ((FRAME_LDS ? wallS[VR_F_SCENE_HI] : p.sceneHi[0]) - o.x) * inv.x;
  const float ty0 = ((FRAME_LDS ? wallS[VR_F_SCENE_LO + 1] : p.sceneLo[1]) - o.y) * inv.y, ty1 = ((FRAME_LDS ? wallS[VR_F_SCENE_HI + 1] : p.sceneHi[1]) - o.y) * inv.y;
  const float tz0 = ((FRAME_LDS ? wallS[VR_F_SCENE_LO + 2] : p.sceneLo[2]) - o.z) * inv.z, tz1 = ((FRAME_LDS ? wallS[VR_F_SCENE_HI + 2] : p.sceneHi[2]) - o.z) * inv.z;
  const float tIn = fmaxf(fmaxf(fminf(tx0, tx1), fminf(ty0, ty1)), fmaxf(fminf(tz0, tz1), tnear));
  const float tOut = fminf(fminf(fmaxf(tx0, tx1), fmaxf(ty0, ty1)), fmaxf(tz0, tz1));
  // tWall: the exact wall test's hit of this ray (or infinity).  A ray that meets a side wall BEFORE it can enter the scene
  // box cannot meet the geometry first (a hit has t >= tIn up to a few ulp: the margin): it stays out of the query's box.
  // Such rays were binned — folded by the boundary condition — with the rays on the far side of the domain, and one of them
  // stretched its wave's box across the whole scene: every packet query of a flat plane that gave up was one of these.
  bool valid = part && tIn <= tOut && !(tWall < tIn * 0.99999f);
  cd.count = 0;
  cd.local = 0ull;
  const float big = 3.0e38f;
  cd.box = false;
  if (!ROUND && !ballot64(valid))
    return true; // nobody reaches the scene box: every ray misses the geometry
  // (Q starts at the ray's origin where that lies inside the box, not at tnear: the neighbour test
  //  accepts any t > 0)
  float tQ = fmaxf(fmaxf(fminf(tx0, tx1), fminf(ty0, ty1)), fmaxf(fminf(tz0, tz1), 0.f));
  float tEnd = tOut;
  if (RELIEF && !(p.debugFlags & 512u)) { // (flag 512: the scene box's clip, for comparison)
    float tA, tB;
    relief_clip(wallS, valid, o, d, tQ, tOut, tA, tB);
    valid = valid && tA <= tB;
    if (!ballot64(valid))
      return true; // no ray's height meets the relief under it
    tQ = tA;
    tEnd = tB;
  }
  const float ax = o.x + d.x * tQ, ay = o.y + d.y * tQ, az = o.z + d.z * tQ;
  const float bx = o.x + d.x * tEnd, by = o.y + d.y * tEnd, bz = o.z + d.z * tEnd;
  float qlx = valid ? fminf(ax, bx) : big, qly = valid ? fminf(ay, by) : big, qlz = valid ? fminf(az, bz) : big;
  float qhx = valid ? fmaxf(ax, bx) : -big, qhy = valid ? fmaxf(ay, by) : -big, qhz = valid ? fmaxf(az, bz) : -big;
  if constexpr (!ROUND)
    wave_minmax6(qlx, qly, qlz, qhx, qhy, qhz);
  const float pad = FRAME_LDS ? wallS[VR_F_PQ_PAD] : p.pqPad;
  qlx -= pad;
  qly -= pad;
  qlz -= pad;
  qhx += pad;
  qhy += pad;
  qhz += pad;
  if constexpr (ROUND) { // the box around the wave's points instead (everything above it is then dead code)
    static_assert(PLANAR && FRAME_LDS && !KEEPQ && !RELIEF, "the round's point is a planar launch's");
    const int pa = __float_as_int(wallS[VR_F_PD_AXIS]);
    int b1, b2;
    planar_in_plane_axes(pa, b1, b2);
    const V3 q = mk(cd.round.qx, cd.round.qy, cd.round.qz);
    const float u = getc(q, b1), v = getc(q, b2);
    const bool in = planar_round_valid(cd.round, u, v, tWall, wallS[VR_F_PR_SB], wallS[VR_F_PR_SB + 1], wallS[VR_F_PR_SB + 2], wallS[VR_F_PR_SB + 3]);
    if (!ballot64(in))
      return true; // nobody's point lies in the scene: every ray misses the geometry
    float ulo = in ? u : big, vlo = in ? v : big, uhi = in ? u : -big, vhi = in ? v : -big;
    wave_minmax4(ulo, vlo, uhi, vhi);
    ulo -= pad;
    vlo -= pad;
    uhi += pad;
    vhi += pad;
    const float alo = wallS[VR_F_PR_QLO], ahi = wallS[VR_F_PR_QHI];
    qlx = pa == 0 ? alo : ulo;
    qhx = pa == 0 ? ahi : uhi;
    qly = pa == 1 ? alo : (pa == 0 ? ulo : vlo);
    qhy = pa == 1 ? ahi : (pa == 0 ? uhi : vhi);
    qlz = pa == 2 ? alo : vlo;
    qhz = pa == 2 ? ahi : vhi;
  }
  if (KEEPQ) {
    cd.box = true;
    if (lane == 0u) {
      cd.rec[VR_PQ_BOX] = mk_u4(__float_as_uint(qlx), __float_as_uint(qly), __float_as_uint(qlz), 0u);
      cd.rec[VR_PQ_BOX + 1] = mk_u4(__float_as_uint(qhx), __float_as_uint(qhy), __float_as_uint(qhz), 0u);
    }
  }
#ifdef VR_DIAG
  unsigned long long pqT0 = __builtin_amdgcn_s_memtime();
#define VR_PQ_MARK(k)                                                                                                  \
  do {                                                                                                                 \
    const unsigned long long now_ = __builtin_amdgcn_s_memtime();                                                      \
    if ((threadIdx.x & 63u) == 0u)                                                                                     \
      phaseT[k] += now_ - pqT0;                                                                                        \
    pqT0 = now_;                                                                                                       \
  } while (0)
#else
#define VR_PQ_MARK(k)
#endif
  // breadth-first search of the 64-ary tree: a frontier entry = {first child, child count | prims flag}
  const float4 *__restrict__ wide = reinterpret_cast<const float4 *>(p.wide);
  const float4 *__restrict__ prims = reinterpret_cast<const float4 *>(p.prims);
  unsigned fFirst = p.wideTopFirst, fCnt = p.wideTopCount;
  unsigned nF = 1;
  const unsigned long long ltMask = (1ull << lane) - 1ull;
  if constexpr (!CACHE) {
  while (!((unsigned)__builtin_amdgcn_readlane((int)fCnt, 0) & VR_WIDE_PRIMS)) {
    unsigned nNext = 0;
    for (unsigned j = 0; j < nF; ++j) {
      const unsigned first = (unsigned)__builtin_amdgcn_readlane((int)fFirst, (int)j);
      const unsigned cnt = (unsigned)__builtin_amdgcn_readlane((int)fCnt, (int)j);
      bool hit = false;
      unsigned cf = 0, cc = 0;
      if (lane < cnt) {
        DIAG(3);
        const float4 a = wide[2 * (size_t)(first + lane)], b = wide[2 * (size_t)(first + lane) + 1];
        hit = all6(a.x <= qhx, b.x >= qlx, a.y <= qhy, b.y >= qly, a.z <= qhz, b.z >= qlz);
        cf = __float_as_uint(a.w);
        cc = __float_as_uint(b.w);
      }
      const unsigned long long m = ballot64(hit);
      const unsigned pos = nNext + (unsigned)__popcll(m & ltMask);
      if (hit && pos < 64u) {
        lst[pos] = cf;
        lst[64u + pos] = cc;
      }
      nNext += (unsigned)__popcll(m);
    }
    if (nNext > p.pqMaxFrontier)
      return false; // (nothing touched yet)
    if (nNext == 0u)
      return true;
    fFirst = lst[lane];
    fCnt = lst[64u + lane];
    nF = nNext;
  }
  } else { // CACHE: the same search with an enlarged box, its frontier kept for the neighbouring rounds
    constexpr unsigned KEEP = VR_PQ_KEEP; // cached leaf nodes (entries lst[0 ..], lst[64 ..]; their boxes: cboxes, 6 floats each)
    const bool caching = p.pqMargin > 0.f && !(fCnt & VR_WIDE_PRIMS);
    bool haveList = false;
    if (caching && lst[39] != 0u) {
      // is the frontier the last search left complete for this round's box?
      const bool inside = qlx >= __uint_as_float(lst[32]) && qly >= __uint_as_float(lst[33]) && qlz >= __uint_as_float(lst[34]) &&
                          qhx <= __uint_as_float(lst[35]) && qhy <= __uint_as_float(lst[36]) && qhz <= __uint_as_float(lst[37]);
      haveList = __builtin_amdgcn_readfirstlane((int)inside) != 0; // (wave-uniform: every operand is)
    }
    if (!haveList) {
      // the search box: the round's own, or — caching — enlarged, so that its frontier serves the neighbouring rounds too
      const float mg = caching ? p.pqMargin : 0.f;
      const float elx = qlx - mg, ely = qly - mg, elz = qlz - mg, ehx = qhx + mg, ehy = qhy + mg, ehz = qhz + mg;
      if (caching && lane == 0u)
        lst[39] = 0u; // (the lists are about to be overwritten; a search that gives up leaves no cache)
      while (!((unsigned)__builtin_amdgcn_readlane((int)fCnt, 0) & VR_WIDE_PRIMS)) {
        unsigned nNext = 0;
        for (unsigned j = 0; j < nF; ++j) {
          const unsigned first = (unsigned)__builtin_amdgcn_readlane((int)fFirst, (int)j);
          const unsigned cnt = (unsigned)__builtin_amdgcn_readlane((int)fCnt, (int)j);
          bool hit = false;
          unsigned cf = 0, cc = 0;
          float4 a = make_float4(0, 0, 0, 0), b = a;
          if (lane < cnt) {
            DIAG(3);
            a = wide[2 * (size_t)(first + lane)];
            b = wide[2 * (size_t)(first + lane) + 1];
            hit = all6(a.x <= ehx, b.x >= elx, a.y <= ehy, b.y >= ely, a.z <= ehz, b.z >= elz);
            cf = __float_as_uint(a.w);
            cc = __float_as_uint(b.w);
          }
          const unsigned long long m = ballot64(hit);
          const unsigned pos = nNext + (unsigned)__popcll(m & ltMask);
          if (hit && pos < 64u) {
            lst[pos] = cf;
            lst[64u + pos] = cc;
            if (caching && pos < KEEP) { // (kept only where this turns out to be the last level)
              cboxes[6u * pos] = a.x, cboxes[6u * pos + 1u] = a.y, cboxes[6u * pos + 2u] = a.z;
              cboxes[6u * pos + 3u] = b.x, cboxes[6u * pos + 4u] = b.y, cboxes[6u * pos + 5u] = b.z;
            }
          }
          nNext += (unsigned)__popcll(m);
        }
        if (nNext > p.pqMaxFrontier) {
          DIAG(14); // (diag: gave up on the frontier)
          return false; // (nothing touched yet)
        }
        if (nNext == 0u && !caching)
          return true;
        fFirst = lst[lane];
        fCnt = lst[64u + lane];
        nF = nNext;
        if (nNext == 0u)
          break; // (nothing meets the enlarged box: an empty frontier, complete for it)
      }
      if (caching) {
        if (nF <= KEEP) {
          if (lane == 0u) {
            lst[32] = __float_as_uint(elx), lst[33] = __float_as_uint(ely), lst[34] = __float_as_uint(elz);
            lst[35] = __float_as_uint(ehx), lst[36] = __float_as_uint(ehy), lst[37] = __float_as_uint(ehz);
            lst[38] = nF;
            lst[39] = 1u;
          }
          haveList = true;
        }
      }
    }
    if (haveList) {
      // the kept leaf nodes that meet THIS round's box (their boxes from LDS: no node load, no dependent trip)
      const unsigned nC = (unsigned)__builtin_amdgcn_readfirstlane((int)lst[38]);
      bool meet = false;
      unsigned f0 = 0, c0 = 0;
      if (lane < nC) {
        // (the six values FIRST, then one combined test: as a chain of && over volatile reads the ISA was six nested
        //  branches, each re-loading the spilled LDS address from scratch behind an s_waitcnt vmcnt(0) — six serial trips
        //  to memory per round of the headline kernel)
        const volatile VR_LDS float *bx = cboxes + 6u * lane;
        const float b0 = bx[0], b1 = bx[1], b2 = bx[2], b3 = bx[3], b4 = bx[4], b5 = bx[5];
        meet = (b0 <= qhx) & (b3 >= qlx) & (b1 <= qhy) & (b4 >= qly) & (b2 <= qhz) & (b5 >= qlz);
        f0 = lst[lane];
        c0 = lst[64u + lane];
      }
      const unsigned long long m = ballot64(meet);
      nF = (unsigned)__popcll(m);
      if (nF == 0u)
        return true;
      if (meet) {
        const unsigned pos = (unsigned)__popcll(m & ltMask);
        lst[16u + pos] = f0;
        lst[80u + pos] = c0;
      }
      fFirst = lst[16u + lane];
      fCnt = lst[80u + lane];
    }
  }
  // last level: the frontier's children are primitives.  Lanes load the RECORDS of a node's
  // (<= 64) primitives, keep those whose bounds meet Q, and every kept record is broadcast from
  // its lane to the whole wave for the exact test: no separate box level, no dependent record fetch.
  // how many candidates are there?  (boxes only, before any exact test: a packet over a relief as
  // deep as it is wide meets dozens of primitives, and for that the slab-test packet or the
  // per-lane walk is cheaper — give up with nothing touched)
  if (nF >= 3u) { // (one or two leaf nodes: the usual case of a compact packet, not worth the extra pass)
    unsigned total = 0;
    for (unsigned j = 0; j < nF; ++j) {
      const unsigned first = (unsigned)__builtin_amdgcn_readlane((int)fFirst, (int)j);
      const unsigned cnt = (unsigned)__builtin_amdgcn_readlane((int)fCnt, (int)j) & 0x7FFFFFFFu;
      bool cand = false;
      if (lane < cnt) {
        const unsigned q = first + lane;
        if (GEO == 0) {
          const float4 r0 = prims[2 * (size_t)q];
          cand = all6(r0.x - r0.w <= qhx, r0.x + r0.w >= qlx, r0.y - r0.w <= qhy, r0.y + r0.w >= qly, r0.z - r0.w <= qhz, r0.z + r0.w >= qlz);
        } else {
          const float4 r0 = prims[4 * (size_t)q], r1 = prims[4 * (size_t)q + 1], r2 = prims[4 * (size_t)q + 2];
          const float v1x = r0.x - r1.x, v1y = r0.y - r1.y, v1z = r0.z - r1.z;
          const float v2x = r0.x + r2.x, v2y = r0.y + r2.y, v2z = r0.z + r2.z;
          cand = fminf(r0.x, fminf(v1x, v2x)) <= qhx && fmaxf(r0.x, fmaxf(v1x, v2x)) >= qlx &&
                 fminf(r0.y, fminf(v1y, v2y)) <= qhy && fmaxf(r0.y, fmaxf(v1y, v2y)) >= qly &&
                 fminf(r0.z, fminf(v1z, v2z)) <= qhz && fmaxf(r0.z, fmaxf(v1z, v2z)) >= qlz;
        }
      }
      total += (unsigned)__popcll(ballot64(cand));
    }
    if (total > p.pqMaxCand) {
      DIAG(15); // (diag: gave up on the candidate count)
      return false;
    }
  }
  // UNIFORM: every candidate has the frame's normal and radius, so the three dot products of the ray with the normal are
  // the same for all of them — the same functions on the same operands as in hit_disc_lds / local_disc_hit_lds, hence
  // the same bits — and the neighbour test's square root becomes a comparison with the frame's threshold
  V3 un = mk(0.f, 0.f, 0.f);
  float uRadius = 0.f, uThresh = 0.f, uDivisor = 0.f, uProd = 0.f, uNro = 0.f;
  if constexpr (UNIFORM) {
    static_assert(GEO == 0 && LEAN, "the uniform-disk tests are forms of the branch-free disc tests");
    un = mk(wallS[VR_F_UD_N], wallS[VR_F_UD_N + 1], wallS[VR_F_UD_N + 2]);
    uRadius = wallS[VR_F_UD_RADIUS];
    uThresh = wallS[VR_F_UD_T];
    uDivisor = edot(d, un);
    uProd = vdot(un, d);
    uNro = vdot(un, o);
  }
  PlanarHit pdH{};
  PlanarLocal pdL{};
  if constexpr (PLANAR && !ROUND) {
    static_assert(UNIFORM, "planar disks are uniform disks");
    const int pa = __float_as_int(wallS[VR_F_PD_AXIS]);
    const float ca = wallS[VR_F_PD_COORD], s = getc(un, pa);
    pdH = planar_hit_round(part, o.x, o.y, o.z, d.x, d.y, d.z, getc(o, pa), tnear, ca, s, uDivisor);
    if (CREDIT)
      pdL = planar_local_round(part, o.x, o.y, o.z, d.x, d.y, d.z, ca, s, uProd, uNro);
  }
  unsigned tests = 0;
  VR_PQ_MARK(14); // (diag: the descent)
  for (unsigned j = 0; j < nF; ++j) {
    const unsigned first = (unsigned)__builtin_amdgcn_readlane((int)fFirst, (int)j);
    const unsigned cnt = (unsigned)__builtin_amdgcn_readlane((int)fCnt, (int)j) & 0x7FFFFFFFu;
    const unsigned q = first + lane; // leaf position (primitive entries of the tree are implicit)
    bool cand = false;
    float4 r0 = make_float4(0, 0, 0, 0), r1 = r0, r2 = r0, r3 = r0;
    if (lane < cnt) {
      DIAG(3);
      if (GEO == 0) {
        r0 = prims[2 * (size_t)q];
        r1 = prims[2 * (size_t)q + 1];
        // a disc lies inside the ball of its radius
        cand = all6(r0.x - r0.w <= qhx, r0.x + r0.w >= qlx, r0.y - r0.w <= qhy, r0.y + r0.w >= qly, r0.z - r0.w <= qhz, r0.z + r0.w >= qlz);
      } else {
        r0 = prims[4 * (size_t)q];
        r1 = prims[4 * (size_t)q + 1];
        r2 = prims[4 * (size_t)q + 2];
        r3 = prims[4 * (size_t)q + 3];
        // vertices v0, v1 = v0 - e1, v2 = v0 + e2 (rounding of the two sums is far inside the pad of Q)
        const float v1x = r0.x - r1.x, v1y = r0.y - r1.y, v1z = r0.z - r1.z;
        const float v2x = r0.x + r2.x, v2y = r0.y + r2.y, v2z = r0.z + r2.z;
        cand = fminf(r0.x, fminf(v1x, v2x)) <= qhx && fmaxf(r0.x, fmaxf(v1x, v2x)) >= qlx &&
               fminf(r0.y, fminf(v1y, v2y)) <= qhy && fmaxf(r0.y, fmaxf(v1y, v2y)) >= qly &&
               fminf(r0.z, fminf(v1z, v2z)) <= qhz && fmaxf(r0.z, fmaxf(v1z, v2z)) >= qlz;
      }
    }
    unsigned long long m = ballot64(cand);
    VR_PQ_MARK(9); // (diag: the candidates' record loads + box tests)
    while (m) {
      const int k = __ffsll((long long)m) - 1;
      m &= m - 1ull;
      if (part) {
        DIAG(4);
      }
      const unsigned qq = first + (unsigned)k;
      float t;
      if constexpr (UNIFORM) { // (the centre and the original id alone are the candidate's own)
        const V3 cc = mk(lane_bcast(r0.x, k), lane_bcast(r0.y, k), lane_bcast(r0.z, k));
        const unsigned orig = (unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(r1.w), k);
        bool ok;
        [[maybe_unused]] bool okLocal = false;
        if constexpr (ROUND) { // (one difference and one square per coordinate for both tests: vr_planar_disks.hpp (1))
          planar_round_cand(cd.round, cc.x, cc.y, cc.z, ok, okLocal);
          t = cd.round.t;
        } else if constexpr (PLANAR) { // (the range tests and `part` are in the round's point: vr_planar_disks.hpp)
          ok = planar_hit_cand(pdH, cc.x, cc.y, cc.z, uRadius);
          t = pdH.t;
        } else {
          ok = part & hit_disc_uniform(o, d, tnear, cc, un, uDivisor, uRadius, t);
        }
        const bool took = hit_update_lds(h, ok, t, orig, qq);
        if (CREDIT) {
          const int c = (int)tests;
          cd.mine = took ? (unsigned)c : cd.mine;
          if ((int)lane == k) { // (the records as crediting reads them: the lane's own r0 / r1)
            cd.rec[c] = mk_u4(qq, __float_as_uint(r0.x), __float_as_uint(r0.y), __float_as_uint(r0.z));
            cd.rec[VR_PQ_NRM + c] = mk_u4(__float_as_uint(r1.x), __float_as_uint(r1.y), __float_as_uint(r1.z), __float_as_uint(r0.w));
          }
          if constexpr (ROUND)
            cd.local |= (unsigned long long)okLocal << c;
          else if constexpr (PLANAR)
            cd.local |= (unsigned long long)planar_local_cand(pdL, cc.x, cc.y, cc.z, uThresh) << c;
          else
            cd.local |= (unsigned long long)(part & local_disc_hit_uniform(o, d, cc, un, uProd, uNro, uThresh)) << c;
          cd.count = tests + 1u;
        }
      } else if (GEO == 0) {
        const float4 c4 = make_float4(lane_bcast(r0.x, k), lane_bcast(r0.y, k), lane_bcast(r0.z, k), lane_bcast(r0.w, k));
        const V3 n = mk(lane_bcast(r1.x, k), lane_bcast(r1.y, k), lane_bcast(r1.z, k));
        const unsigned orig = (unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(r1.w), k);
        bool ok, took;
        if constexpr (LEAN) { // (the absorbing flat-scene kernel: the branch-free forms, see hit_disc_lds)
          ok = hit_disc_lds(o, d, tnear, c4, n, t);
          took = hit_update_lds(h, part & ok, t, orig, qq);
        } else {
          ok = hit_disc(o, d, tnear, c4, n, t);
          took = hit_update(h, part && ok, t, orig, qq);
        }
        if (CREDIT) {
          const int c = (int)tests;
          cd.mine = took ? (unsigned)c : cd.mine;
          if ((int)lane == k) { // (the lane that loaded the record files it: its r0 / r1 are the broadcast c4 / n)
            cd.rec[c] = mk_u4(qq, __float_as_uint(r0.x), __float_as_uint(r0.y), __float_as_uint(r0.z));
            cd.rec[VR_PQ_NRM + c] = mk_u4(__float_as_uint(r1.x), __float_as_uint(r1.y), __float_as_uint(r1.z), __float_as_uint(r0.w));
          }
          // (a wave-wide early out between the cheap sign tests and the division / distance part of
          //  these two tests was measured: the extra votes and branches cost more than they save)
          if constexpr (LEAN)
            cd.local |= (unsigned long long)(part & local_disc_hit_lds(o, d, c4, n)) << c;
          else if (part && local_disc_hit(o, d, c4, n))
            cd.local |= 1ull << c;
          cd.count = tests + 1u;
        }
      } else {
        const V3 v0 = mk(lane_bcast(r0.x, k), lane_bcast(r0.y, k), lane_bcast(r0.z, k));
        const V3 e1 = mk(lane_bcast(r1.x, k), lane_bcast(r1.y, k), lane_bcast(r1.z, k));
        const V3 e2 = mk(lane_bcast(r2.x, k), lane_bcast(r2.y, k), lane_bcast(r2.z, k));
        const V3 Ng = mk(lane_bcast(r3.x, k), lane_bcast(r3.y, k), lane_bcast(r3.z, k));
        const unsigned orig = (unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(r0.w), k);
        const bool ok = hit_tri(o, d, tnear, v0, e1, e2, Ng, t);
        hit_update(h, part && ok, t, orig, qq);
      }
      if (++tests > 2u * p.pqMaxCand) {
        DIAG(10); // (diag: gave up in the exact tests)
        return false; // (only reachable with <= 2 leaf nodes: the hits found so far are real, the walk goes on from them)
      }
    }
    VR_PQ_MARK(15); // (diag: the exact tests)
  }
  return true;
}

// ---------------------------------------------------------------------------
// The packet query of a LATTICE cloud (trace_kernel MODE_ABSORB_FLAT_LATTICE; vr_planar_lattice.hpp has the table and
// the argument): the contract of pq_hit_packet<... ROUND> — the same inputs, the same h, cd.rec, cd.local, cd.count and
// cd.mine behind it, false with nothing touched — without the search.  The round's box is the parent's (planar_round_valid,
// wave_minmax4 of the plane hits, the pad); the disks that can meet it are the lattice points of an index window that
// follows from the box, lane l owns cell l of the window: one table word, then the disk's two record words, then THE
// PARENT'S ball-box filter on those record bits.  The ballot of that filter feeds the parent's candidate loop; the leaf
// position of a candidate comes from its owning lane.  No tree, no frontier lists, no leaf-node boxes in LDS.
// Gives up (false, nothing touched) where the window has more cells than the wave has lanes, or more candidates pass the
// filter than 2 * pqMaxCand (the parent's bound on the exact tests of a round; VR_PQ_CANDS holds that many records).
// Every table index is formed from window indices clamped to the table (lattice_axis_window) by a lane inside the window,
// every record index is a table word that is not VR_LATTICE_EMPTY: the table's kernel wrote leaf positions below numPrims.
// ---------------------------------------------------------------------------
template <bool CREDIT>
__device__ __forceinline__ bool pq_hit_lattice(const TraceParams &p, HitRec &h, PqCands &cd, const float *__restrict__ wallS,
                                               float tWall VR_DIAG_ARGS) {
  const unsigned lane = threadIdx.x & 63u;
  cd.count = 0;
  cd.local = 0ull;
  cd.box = false;
  const float big = 3.0e38f;
  const int pa = __float_as_int(wallS[VR_F_PD_AXIS]);
  int b1, b2;
  planar_in_plane_axes(pa, b1, b2);
  const V3 q = mk(cd.round.qx, cd.round.qy, cd.round.qz);
  const float u = getc(q, b1), v = getc(q, b2);
  const bool in = planar_round_valid(cd.round, u, v, tWall, wallS[VR_F_PR_SB], wallS[VR_F_PR_SB + 1], wallS[VR_F_PR_SB + 2], wallS[VR_F_PR_SB + 3]);
  if (!ballot64(in))
    return true; // nobody's point lies in the scene: every ray misses the geometry
  float ulo = in ? u : big, vlo = in ? v : big, uhi = in ? u : -big, vhi = in ? v : -big;
  wave_minmax4(ulo, vlo, uhi, vhi);
  const float pad = wallS[VR_F_PQ_PAD];
  ulo -= pad;
  vlo -= pad;
  uhi += pad;
  vhi += pad;
#ifdef VR_DIAG
  unsigned long long pqT0 = __builtin_amdgcn_s_memtime();
#endif
  // the window of lattice points around the box (wave-uniform: every operand is)
  const int n1 = __float_as_int(wallS[VR_F_PL_N1]), n2 = __float_as_int(wallS[VR_F_PL_N2]);
  const float invD = wallS[VR_F_PL_INVD], reach = wallS[VR_F_PL_REACH];
  int i0, i1, j0, j1;
  lattice_axis_window(ulo, uhi, wallS[VR_F_PL_PHASE1], invD, reach, n1, i0, i1);
  lattice_axis_window(vlo, vhi, wallS[VR_F_PL_PHASE2], invD, reach, n2, j0, j1);
  i0 = __builtin_amdgcn_readfirstlane(i0);
  i1 = __builtin_amdgcn_readfirstlane(i1);
  j0 = __builtin_amdgcn_readfirstlane(j0);
  j1 = __builtin_amdgcn_readfirstlane(j1);
  const int w = i1 - i0 + 1, rows = j1 - j0 + 1;
  if (w <= 0 || rows <= 0)
    return true; // no lattice point near the box: every ray misses the geometry
  if (w > VR_LATTICE_WINDOW || rows > VR_LATTICE_WINDOW || w * rows > VR_LATTICE_WINDOW) {
    DIAG(14); // (diag: gave up on the window)
    return false; // (nothing touched yet)
  }
  const float qlx = pa == 0 ? wallS[VR_F_PR_QLO] : ulo, qhx = pa == 0 ? wallS[VR_F_PR_QHI] : uhi;
  const float qly = pa == 1 ? wallS[VR_F_PR_QLO] : (pa == 0 ? ulo : vlo), qhy = pa == 1 ? wallS[VR_F_PR_QHI] : (pa == 0 ? uhi : vhi);
  const float qlz = pa == 2 ? wallS[VR_F_PR_QLO] : vlo, qhz = pa == 2 ? wallS[VR_F_PR_QHI] : vhi;
  typedef const __attribute__((address_space(1))) unsigned *GlobalU32;
  const GlobalU32 table = reinterpret_cast<GlobalU32>(frame_addr(wallS, VR_F_PL_PTR_LO));
  const float4 *__restrict__ prims = reinterpret_cast<const float4 *>(p.prims);
  unsigned pos = VR_LATTICE_EMPTY; // this lane's disk: its leaf position
  bool cand = false;
  float4 r0 = make_float4(0, 0, 0, 0), r1 = r0;
  if ((int)lane < w * rows) {
    int col, row;
    lattice_lane_cell((int)lane, w, __builtin_amdgcn_rcpf((float)w), col, row);
    // (inside the window for every rounding of the reciprocal: the clamp costs two instructions, a load outside the table a fault)
    col = col < 0 ? 0 : (col >= w ? w - 1 : col);
    row = row < 0 ? 0 : (row >= rows ? rows - 1 : row);
    pos = table[(unsigned)(j0 + row) * (unsigned)n1 + (unsigned)(i0 + col)];
    if (pos != VR_LATTICE_EMPTY) {
      DIAG(3);
      r0 = prims[2 * (size_t)pos];
      r1 = prims[2 * (size_t)pos + 1];
      // a disc lies inside the ball of its radius (the parent's filter, on the same box)
      cand = all6(r0.x - r0.w <= qhx, r0.x + r0.w >= qlx, r0.y - r0.w <= qhy, r0.y + r0.w >= qly, r0.z - r0.w <= qhz, r0.z + r0.w >= qlz);
    }
  }
  unsigned long long m = ballot64(cand);
  if ((unsigned)__popcll(m) > 2u * p.pqMaxCand) {
    DIAG(15); // (diag: gave up on the candidate count)
    return false; // (nothing touched yet)
  }
#ifdef VR_DIAG
  {
    const unsigned long long now_ = __builtin_amdgcn_s_memtime();
    if (lane == 0u)
      phaseT[9] += now_ - pqT0; // (diag: the window, the candidates' record loads + box tests)
    pqT0 = now_;
  }
#endif
  unsigned tests = 0;
  while (m) {
    const int k = __ffsll((long long)m) - 1;
    m &= m - 1ull;
    DIAG(4);
    const unsigned qq = (unsigned)__builtin_amdgcn_readlane((int)pos, k);
    const V3 cc = mk(lane_bcast(r0.x, k), lane_bcast(r0.y, k), lane_bcast(r0.z, k));
    const unsigned orig = (unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(r1.w), k);
    bool ok, okLocal;
    planar_round_cand(cd.round, cc.x, cc.y, cc.z, ok, okLocal); // (one difference and one square per coordinate for both tests)
    const bool took = hit_update_lds(h, ok, cd.round.t, orig, qq);
    if (CREDIT) {
      const int c = (int)tests;
      cd.mine = took ? (unsigned)c : cd.mine;
      if ((int)lane == k) { // (the records as crediting reads them: the lane's own r0 / r1)
        cd.rec[c] = mk_u4(qq, __float_as_uint(r0.x), __float_as_uint(r0.y), __float_as_uint(r0.z));
        cd.rec[VR_PQ_NRM + c] = mk_u4(__float_as_uint(r1.x), __float_as_uint(r1.y), __float_as_uint(r1.z), __float_as_uint(r0.w));
      }
      cd.local |= (unsigned long long)okLocal << c;
      cd.count = tests + 1u;
    }
    ++tests;
  }
#ifdef VR_DIAG
  {
    const unsigned long long now_ = __builtin_amdgcn_s_memtime();
    if (lane == 0u)
      phaseT[15] += now_ - pqT0; // (diag: the exact tests)
  }
#endif
  return true;
}

// ---------------------------------------------------------------------------
// The packet query of a lattice cloud whose disks are small against the pitch (trace_kernel MODE_ABSORB_FLAT_LATTICE_LANES;
// vr_planar_lattice.hpp "four corners per lane" has the rule and the argument): pq_hit_lattice's box and window, then NO
// candidate loop and no give-up (a window of more than 64 cells: the direct form, in the function).  Lane l files the disk of window cell l — {leaf position, centre} in record l of
// the wave's LDS records, its original id in word l behind them, VR_LATTICE_EMPTY where the cell has none — and every lane
// tests the four disks at the corners of ITS point's cell: planar_round_cand on the record's bits, hit_update_lds with the
// record's id and leaf position, as the candidate loop does.  A disk that accepts a lane's point is one of its four corners
// (the rule), and for a lane whose point is in the round's box it lies inside the window (the window's argument: it passes
// the parent's ball-box filter); the other lanes accept nothing that counts (a wall comes first, or the point lies outside
// the scene).  So each lane sees every disk that pq_hit_lattice's loop would have let it accept, and the closest-hit rule
// does not depend on the others.  No ball-box filter, no ballot, no give-up on the candidate count: always true.
// Behind it: h; cd.mine = which of the four corners is the lane's closest hit; cd.local = bit k: the lane's ray passes the
// neighbour test on corner k; cd.slots = the four window slots, a byte each (VR_PQ_NO_SLOT: a corner outside the window);
// cd.count = 0.  The wave's records: VR_PQ_LANE_IDS .. hold the 64 id words, VR_PQ_LANE_CNT .. the 64 counters of the
// crediting (trace_kernel), all inside the VR_PQ_RECORDS records the wave has anyway.
// Every LDS index is a window slot (lattice_window_slot: below w * rows <= 64) or 0, every table index is formed as in
// pq_hit_lattice, and the cell's indices pass through lattice_lane_corner's clamp in float.
// ---------------------------------------------------------------------------
constexpr unsigned VR_PQ_NO_SLOT = 0xFFu;
constexpr unsigned VR_PQ_LANE_IDS = 64, VR_PQ_LANE_CNT = 80; // (records: 16 of them hold 64 words)
static_assert(VR_PQ_LANE_CNT + 16u <= VR_PQ_RECORDS && VR_LATTICE_WINDOW == 64, "the wave's records hold the lanes' tables");
template <bool CREDIT>
__device__ __forceinline__ bool pq_hit_lattice_lanes(const TraceParams &p, HitRec &h, PqCands &cd, const float *__restrict__ wallS,
                                                     float tWall VR_DIAG_ARGS) {
  const unsigned lane = threadIdx.x & 63u;
  cd.count = 0;
  cd.local = 0ull;
  cd.box = false;
  const float big = 3.0e38f;
  const int pa = __float_as_int(wallS[VR_F_PD_AXIS]);
  int b1, b2;
  planar_in_plane_axes(pa, b1, b2);
  const V3 q = mk(cd.round.qx, cd.round.qy, cd.round.qz);
  const float u = getc(q, b1), v = getc(q, b2);
  const bool in = planar_round_valid(cd.round, u, v, tWall, wallS[VR_F_PR_SB], wallS[VR_F_PR_SB + 1], wallS[VR_F_PR_SB + 2], wallS[VR_F_PR_SB + 3]);
  if (!ballot64(in))
    return true; // nobody's point lies in the scene: every ray misses the geometry
  float ulo = in ? u : big, vlo = in ? v : big, uhi = in ? u : -big, vhi = in ? v : -big;
  wave_minmax4(ulo, vlo, uhi, vhi);
  const float pad = wallS[VR_F_PQ_PAD];
  ulo -= pad;
  vlo -= pad;
  uhi += pad;
  vhi += pad;
#ifdef VR_DIAG
  unsigned long long pqT0 = __builtin_amdgcn_s_memtime();
#endif
  // the window of lattice points around the box (wave-uniform: every operand is)
  const int n1 = __float_as_int(wallS[VR_F_PL_N1]), n2 = __float_as_int(wallS[VR_F_PL_N2]);
  const float invD = wallS[VR_F_PL_INVD], reach = wallS[VR_F_PL_REACH];
  const float phase1 = wallS[VR_F_PL_PHASE1], phase2 = wallS[VR_F_PL_PHASE2];
  int i0, i1, j0, j1;
  lattice_axis_window(ulo, uhi, phase1, invD, reach, n1, i0, i1);
  lattice_axis_window(vlo, vhi, phase2, invD, reach, n2, j0, j1);
  i0 = __builtin_amdgcn_readfirstlane(i0);
  i1 = __builtin_amdgcn_readfirstlane(i1);
  j0 = __builtin_amdgcn_readfirstlane(j0);
  j1 = __builtin_amdgcn_readfirstlane(j1);
  const int w = i1 - i0 + 1, rows = j1 - j0 + 1;
  if (w <= 0 || rows <= 0)
    return true; // no lattice point near the box: every ray misses the geometry
  typedef const __attribute__((address_space(1))) unsigned *GlobalU32;
  const GlobalU32 table = reinterpret_cast<GlobalU32>(frame_addr(wallS, VR_F_PL_PTR_LO));
  const float4 *__restrict__ prims = reinterpret_cast<const float4 *>(p.prims);
  if (w > VR_LATTICE_WINDOW || rows > VR_LATTICE_WINDOW || w * rows > VR_LATTICE_WINDOW) {
    // The window does not fit the wave (a round that holds a ray folded in from the far side of the domain): the DIRECT
    // form.  The rule needs no window — a disk that accepts a lane's point is a corner of its cell, wherever the other
    // lanes' points lie — so each lane reads its four table words and records from global memory: a corner outside the
    // table is no candidate, the table index of one inside is below n1 n2, and an absent corner reads word 0 / record 0,
    // which exist.  The same tests on the same record bits as the tree packet and the walk make, the same tie rule: the
    // hits are theirs.  Behind it: cd.count = 1 (wave-uniform: the decision is), record l of the wave = lane l's four
    // leaf positions (VR_LATTICE_EMPTY: none) for the crediting, cd.local as below.
    DIAG(14); // (diag: the window did not fit)
    const int di = lattice_lane_corner(u, phase1, invD, n1), dj = lattice_lane_corner(v, phase2, invD, n2);
    unsigned ps[4], loc = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      DIAG(4);
      const int i = di + (k & 1), j = dj + (k >> 1);
      const bool inT = (i >= 0) & (i < n1) & (j >= 0) & (j < n2);
      const unsigned pos = table[inT ? (unsigned)j * (unsigned)n1 + (unsigned)i : 0u];
      const bool present = inT & (pos != VR_LATTICE_EMPTY);
      const size_t rp = present ? (size_t)pos : (size_t)0;
      const float4 r0 = prims[2 * rp];
      const unsigned orig = __float_as_uint(prims[2 * rp + 1].w);
      bool ok, okLocal;
      planar_round_cand(cd.round, r0.x, r0.y, r0.z, ok, okLocal);
      hit_update_lds(h, ok & present, cd.round.t, orig, pos);
      loc |= (unsigned)(okLocal & present) << k;
      ps[k] = present ? pos : VR_LATTICE_EMPTY;
    }
    if (CREDIT) {
      cd.rec[lane] = mk_u4(ps[0], ps[1], ps[2], ps[3]);
      cd.local = (unsigned long long)loc;
      cd.count = 1u;
      cd.slots = 0u;
    }
    return true;
  }
  VR_LDS unsigned *const ids = (VR_LDS unsigned *)(cd.rec + VR_PQ_LANE_IDS);
  { // lane l files the disk of window cell l
    unsigned pos = VR_LATTICE_EMPTY;
    float4 r0 = make_float4(0, 0, 0, 0);
    unsigned orig = 0u;
    if ((int)lane < w * rows) {
      int col, row;
      lattice_lane_cell((int)lane, w, __builtin_amdgcn_rcpf((float)w), col, row);
      // (inside the window for every rounding of the reciprocal: the clamp costs two instructions, a load outside the table a fault)
      col = col < 0 ? 0 : (col >= w ? w - 1 : col);
      row = row < 0 ? 0 : (row >= rows ? rows - 1 : row);
      pos = table[(unsigned)(j0 + row) * (unsigned)n1 + (unsigned)(i0 + col)];
      if (pos != VR_LATTICE_EMPTY) {
        DIAG(3);
        r0 = prims[2 * (size_t)pos];
        orig = __float_as_uint(prims[2 * (size_t)pos + 1].w);
      }
    }
    // (the lane made an opaque value here, so that the record's address and the lane's float are recomputed per round and
    //  not hoisted and spilled — no scratch left in the kernel — was built and measured: trace 2.44 ms against 2.38 ms)
    cd.rec[lane] = mk_u4(pos, __float_as_uint(r0.x), __float_as_uint(r0.y), __float_as_uint(r0.z));
    ids[lane] = orig;
  }
  __builtin_amdgcn_wave_barrier();
#ifdef VR_DIAG
  {
    const unsigned long long now_ = __builtin_amdgcn_s_memtime();
    if (lane == 0u)
      phaseT[9] += now_ - pqT0; // (diag: the window, the cells' record loads, their filing)
    pqT0 = now_;
  }
#endif
  // the four corners of this lane's cell.  (Every lane: one whose thresholds are both 0 accepts nothing, and a branch
  // around it would be exec bookkeeping for the lanes of a wave that nearly all take part.)
  const int ci = lattice_lane_corner(u, phase1, invD, n1), cj = lattice_lane_corner(v, phase2, invD, n2);
  unsigned slots = 0u, local = 0u;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    DIAG(4);
    const int s = lattice_window_slot(ci + (k & 1), cj + (k >> 1), i0, i1, j0, j1);
    const unsigned sl = s < 0 ? 0u : (unsigned)s; // (slot 0 is a cell of every window: its record is this round's)
    const U4 cr = cd.rec[sl];
    const unsigned orig = ids[sl];
    const bool present = (s >= 0) & (cr.x != VR_LATTICE_EMPTY);
    bool ok, okLocal;
    planar_round_cand(cd.round, __uint_as_float(cr.y), __uint_as_float(cr.z), __uint_as_float(cr.w), ok, okLocal);
    const bool took = hit_update_lds(h, ok & present, cd.round.t, orig, cr.x);
    if (CREDIT) {
      cd.mine = took ? (unsigned)k : cd.mine;
      local |= (unsigned)(okLocal & present) << k;
      slots |= (s < 0 ? VR_PQ_NO_SLOT : (unsigned)s) << (8 * k);
    }
  }
  cd.local = (unsigned long long)local;
  cd.slots = slots;
#ifdef VR_DIAG
  {
    const unsigned long long now_ = __builtin_amdgcn_s_memtime();
    if (lane == 0u)
      phaseT[15] += now_ - pqT0; // (diag: the exact tests)
  }
#endif
  return true;
}

} // namespace vr
