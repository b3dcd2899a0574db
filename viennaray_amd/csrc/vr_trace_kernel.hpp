// vr_trace_kernel.hpp — everything the trace kernel is made of: the crediting helpers, the boundary state machine's
// processHit, the height-field test, the tuning knobs and trace_kernel itself (the round structure is described in
// vr_trace.hip; the modes in vr_types.hpp, enum TraceMode).  Included by the library's table of kernels (vr_trace.hip),
// by a run-time particle module (vr_modules.hpp) and by the diagnostic kernels that share its helpers (vr_diag.hip).
//
// tools/salu_inventory.py finds the phases of a round by the `// ---- ` marker comments of the kernel body: their texts
// are listed there, and each must stay unique and in order.
#pragma once
#include "vr_device.hpp"
#include "vr_particles.hpp"

namespace vr {

// fixed-point weight: 2^40 per unit (order-independent integer accumulation)
__device__ __forceinline__ u64 weight_fx(float w) { return (u64)((double)w * 1099511627776.0 + 0.5); }
// flux statistics: the square of a credited value, taken in double and quantised like the value itself
__device__ __forceinline__ u64 weight_sq_fx(float w) { return (u64)((double)w * (double)w * 1099511627776.0 + 0.5); }

__device__ __forceinline__ unsigned long long wave_sum(unsigned v) {
  unsigned long long s = v;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    s += __shfl_down(s, off, 64);
  return s;
}

// Credit `wfx` to accumulator `pos` for every lane with `cond`; lanes of the wave that
// credit the same accumulator with the same weight are merged into one atomic
// (sorted rays: a wavefront's hits fall on a handful of disks).
__device__ __forceinline__ void credit_aggregated(unsigned long long *acc, bool cond, unsigned pos, u64 wfx) {
  unsigned long long todo = ballot64(cond);
  const unsigned lane = threadIdx.x & 63u;
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const unsigned P = __shfl(pos, leader, 64);
    const unsigned wlo = __shfl((unsigned)(wfx & 0xFFFFFFFFull), leader, 64);
    const unsigned whi = __shfl((unsigned)(wfx >> 32), leader, 64);
    const u64 W = ((u64)whi << 32) | wlo;
    const unsigned long long same = ballot64(cond && pos == P && wfx == W);
    if ((int)lane == leader)
      atomicAdd(&acc[P], W * (u64)__popcll(same));
    todo &= ~same;
  }
}

// Every lane of the wave adds `wfx` (0: nothing) to the SAME accumulator `pos`: one integer wave sum (exact, order
// independent) and one atomic.  Must be reached by the whole wave.
__device__ __forceinline__ void credit_wave_sum(unsigned long long *acc, unsigned pos, u64 wfx) {
  u64 s = wfx;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    s += (u64)__shfl_down((unsigned long long)s, off, 64);
  if ((threadIdx.x & 63u) == 0u && s)
    atomicAdd(&acc[pos], s);
}

__device__ __forceinline__ unsigned long long bcast64(unsigned long long v) {
  unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)(v & 0xFFFFFFFFull));
  unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return ((unsigned long long)hi << 32) | lo;
}

// Boundary::processHit (rayBoundary.hpp:29-127): what a hit of wall triangle `prim` at hitPoint does to the
// ray.  Shared by trace_kernel and the debug entry point that checks the reference's boundaryHit known answers.
template <int D>
__device__ __forceinline__ void process_boundary_hit(const TraceParams &p, const float *__restrict__ wallS, unsigned prim,
                                                     const V3 &hitPoint, V3 &org, V3 &rayDirection, V3 &dir,
                                                     bool &active) {
  const float *w = wallS + 12 * prim;
  V3 ng = mk(w[9], w[10], w[11]);
  if (vdot(dir, ng) > 0.f) { // back side: pass through
    org = hitPoint;
    return;
  }
  int bc, axis;
  bool minWall;
  if (D == 2 || prim <= 3u) {
    bc = p.bc0;
    axis = p.firstDir;
    minWall = prim <= 1u;
  } else {
    bc = p.bc1;
    axis = p.secondDir;
    minWall = prim <= 5u;
  }
  if (bc == 0) { // REFLECTIVE, rayBoundary.hpp:261-271
    vnormalize(ng);
    rayDirection = reflect_specular(rayDirection, ng);
    dir = project_dir<D>(rayDirection);
    org = hitPoint;
  } else if (bc == 1) { // PERIODIC: wrap to the opposite face
    org = hitPoint;
    const bool first = (D == 2 || prim <= 3u);
    const float wrapTo = first ? (minWall ? p.hi1 : p.lo1) : (minWall ? p.hi2 : p.lo2);
    setc(org, axis, wrapTo);
  } else { // IGNORE
    active = false;
  }
}

// material id of ORIGINAL primitive `origId` for a stateful model's hooks (the frame's VR_F_MAT_*; none set: 0)
__device__ __forceinline__ int material_of(const float *wallS, unsigned origId) {
  const int *ids = reinterpret_cast<const int *>(frame_addr(wallS, VR_F_MAT_LO));
  return ids ? ids[origId] : 0;
}

// "Segments that rise clear" (trace_kernel): does the height field over the source plane (HeightFieldParams, the launch
// frame's VR_F_HF_*) say that a ray starting at `org` cannot meet the geometry?  It is above its tile's height — the highest
// point of anything in the tile or its eight neighbours — from tnear on, and rises above the whole scene before it has
// travelled a tile sideways.  One look-up, no loop.
template <int D>
__device__ __forceinline__ bool rises_clear(const float *__restrict__ wallS, const V3 &org, const V3 &dir, float tnear) {
  const int hnx = __float_as_int(wallS[VR_F_HF_NX]);
  if (hnx <= 0)
    return false;
  const int ax = __float_as_int(wallS[VR_F_RAYDIR]), a1 = __float_as_int(wallS[VR_F_FIRSTDIR]), a2 = __float_as_int(wallS[VR_F_SECONDDIR]);
  const float sgn = wallS[VR_F_HF_SIGN];
  const float up = sgn * getc(dir, ax);
  if (!(up > 0.f))
    return false;
  const float hz = sgn * getc(org, ax);
  const float invT = wallS[VR_F_HF_INVT];
  const int hny = __float_as_int(wallS[VR_F_HF_NY]);
  int ix = (int)floorf((getc(org, a1) - wallS[VR_F_HF_LO1]) * invT);
  ix = ix < 0 ? 0 : (ix >= hnx ? hnx - 1 : ix);
  int iy = 0;
  float d2 = 0.f;
  if (D == 3) {
    iy = (int)floorf((getc(org, a2) - wallS[VR_F_HF_LO2]) * invT);
    iy = iy < 0 ? 0 : (iy >= hny ? hny - 1 : iy);
    d2 = getc(dir, a2);
  }
  typedef const __attribute__((address_space(1))) float *GlobalF;
  const GlobalF field = reinterpret_cast<GlobalF>(((unsigned long long)__float_as_uint(wallS[VR_F_HF_PTR_HI]) << 32) |
                                                  __float_as_uint(wallS[VR_F_HF_PTR_LO]));
  const float height = field[iy * hnx + ix];
  const float d1 = getc(dir, a1);
  const float tTop = fmaxf(wallS[VR_F_HF_TOP] - hz, 0.f) / up; // where the ray passes the top of the scene box
  return hz + up * tnear > height && tTop * sqrtf(d1 * d1 + d2 * d2) <= 0.99f * wallS[VR_F_HF_TILE];
}

// ---------------------------------------------------------------------------
// trace_kernel
//   ABSORB: every hit absorbs the whole weight (sticking >= 1 everywhere), so
//   nothing after the first surface hit is observable and the reflection /
//   roulette code (and its RNG) is compiled out.
// ---------------------------------------------------------------------------
// The modes (template parameter MODE_): enum TraceMode, vr_types.hpp.
// (SGPR budget: 256-thread blocks per CU = min(8, 800 / (ceil(sgpr/16)*16 + 16)) on gfx950,
//  MI355X_MICROARCH.md; 80 keeps 8 blocks resident)
// The tuning knobs (the waves per SIMD of each mode: VR_*_WAVES next to mode_traits, vr_types.hpp):
#ifndef VR_FLAT_ORDERED
#define VR_FLAT_ORDERED 0  // MODE_GENERAL_FLAT walks like MODE_ABSORB_FLAT: the escape-link walk, no carry-over (1: the ordered pair walk).  It runs
                           // only on scenes whose box is thin (vr_prepare.cpp: flatScene), where a wave walks in the 5 % of its
                           // rounds whose query gives up; without the walk's 12 KB of LDS stack and ~10 VGPRs the kernel
                           // takes 6 waves per SIMD: C2 0.1 10.9 -> 10.0 ms.  (Forced onto a scene with relief
                           // — VR_GENERAL_FLAT=1 — it is 15 - 30 % slower than with the ordered walk at 5 waves.)
#endif
#ifndef VR_PQ_CACHE
#define VR_PQ_CACHE 1      // flat-scene kernels: the packet query's frontier serves the neighbouring rounds (pq_hit_packet CACHE)
#endif
#ifndef VR_PQ_WALLS_FIRST
#define VR_PQ_WALLS_FIRST 1 // flat-scene kernels: a ray that meets a side wall before the scene box stays out of the packet query's box
#endif
#ifndef VR_PQ_CACHE_RELIEF
#define VR_PQ_CACHE_RELIEF 1 // ... in the relief kernels MODE_ABSORB_RELIEF / MODE_GENERAL_RELIEF too
#endif
constexpr unsigned VR_SPILL_BLOCK = 64u; // records of the spill queue a wave reserves at a time (TraceParams::spillRec)
// the unused records [used, VR_SPILL_BLOCK) of a wave's block marked empty (word 11 = ~0: no ray)
__device__ __forceinline__ void spill_pad(const TraceParams &p, unsigned base, unsigned used, unsigned lane) {
  if (used < VR_SPILL_BLOCK && lane >= used)
    reinterpret_cast<float4 *>(p.spillRec)[4 * (size_t)(base + lane) + 2] = make_float4(0.f, 0.f, 0.f, __uint_as_float(0xFFFFFFFFu));
}
// the catalogue's set this translation unit instantiates from (trace_kernel_exists, vr_types.hpp)
#ifdef VR_USER_MODULE
constexpr KernelSet VR_KERNEL_SET = KERNELS_MODULE;
#else
constexpr KernelSet VR_KERNEL_SET = KERNELS_LIBRARY;
#endif
template <int D, int GEO, int PARTICLE, int MODE_>
__global__ __launch_bounds__(VR_BLOCK) __attribute__((amdgpu_num_sgpr(80)))
__attribute__((amdgpu_waves_per_eu(mode_traits(MODE_).waves, mode_traits(MODE_).waves))) void
trace_kernel(const TraceParams p) {
  constexpr ModeTraits T = mode_traits(MODE_); // (what the mode is: vr_types.hpp)
  constexpr bool SMALL = T.small;
  constexpr bool RELIEF = T.relief;
  constexpr bool RESUME = T.resume;
  constexpr bool LATTICE_LANES = T.latticeLanes; // (... each lane testing the four disks at the corners of its point's cell: pq_hit_lattice_lanes)
  constexpr bool PLANAR_LATTICE = T.lattice; // (... with the round's candidates from the lattice table: pq_hit_lattice, vr_planar_lattice.hpp)
  static_assert(!T.lattice || T.planarRound, "the lattice table serves the one-point-per-round kernel");
  constexpr bool PLANAR_ROUND = T.planarRound; // (... with the plane hit as the round's one point: pq_hit_packet ROUND, wall-free rounds)
  constexpr bool PLANAR = T.planar; // (... with its PLANAR candidate tests, which are UNIFORM ones)
  constexpr bool UNIFORM = T.uniform; // (MODE_ABSORB_FLAT with pq_hit_packet's UNIFORM candidate tests)
  constexpr int MODE = T.base;
  constexpr bool FRAME_LDS = MODE == MODE_ABSORB_FLAT; // (the wall / scene-box frame from LDS: hit_walls_lds, vr_intersect.hpp)
  // (the scalar diet of the absorbing flat-scene kernel — branch-free candidate tests, lane-parallel crediting — in three
  //  dimensions only: the 2-D instantiations answered it with vector spills, DESIGN_APPENDIX A)
  constexpr bool LEAN = MODE == MODE_ABSORB_FLAT && D == 3 && GEO == 0 && PARTICLE < P_EXT;
  static_assert(trace_kernel_exists(VR_KERNEL_SET, D, GEO, PARTICLE, MODE_), "not a kernel of the catalogue (trace_kernel_exists, vr_types.hpp)");
  static_assert(!UNIFORM || LEAN, "the uniform-disk variants are written for the LEAN kernel");
  constexpr bool FOLLOW = MODE == MODE_GENERAL_FLAT;    // (follow-up segments inside the round of a packet query: end of the round)
  constexpr bool ABSORB = MODE == MODE_ABSORB_FLAT || MODE == MODE_ABSORB;
  // PARTICLE 0 / 1: DiffuseParticle / SpecularParticle compiled in.  PARTICLE 2 (P_EXT): the
  // extended kernel — particle kind, data labels, WDIST crediting and mean-free-path scattering
  // decided at run time from TraceParams (vr_particles.hpp)
  constexpr bool EXT = PARTICLE >= P_EXT;           // (P_EXT, P_EXT_FULL and their twins with flux statistics)
  constexpr bool EXT_FULL = PARTICLE == P_EXT_FULL || PARTICLE == P_EXT_FULL_STATS; // ... with the coned-cosine model, WDIST crediting and the mean free path
  // Flux statistics (vr_set_flux_statistics): every credit(0, v) of the model's collide also adds weight_sq_fx(v) to plane
  // numData (the sum of squares, 2^-40 per unit like the flux) and 1 to plane numData + 1 (the hit count, in units of ONE).
  // Integer sums like the flux: exact, whatever the grid, the batch split or the rank count.
  constexpr bool STATS = PARTICLE == P_EXT_STATS || PARTICLE == P_EXT_FULL_STATS;
  // per-ray state words of a stateful model (vr_particles.hpp): only a module compiled around one has them (0 in the library)
  constexpr int SW = EXT_FULL ? Particles::stateWords : 0;
  // packet-query rounds credit disks wave-uniformly from the candidate list (pq_credit) instead of
  // walking the neighbour CSR per lane
  constexpr bool PQ_CREDIT = GEO == 0 && !EXT_FULL && (MODE == MODE_ABSORB_FLAT || MODE == MODE_GENERAL_FLAT);
  PqCands cands;
  cands.local = 0ull;
  cands.count = 0u;
  cands.box = false;
  cands.mine = 0u;
  cands.rec = nullptr;
  // CARRY: lanes whose BVH walk is still under way when most of the wave is done keep
  // their cursor over the state-machine / refill phase (see the round structure below).
  // The absorbing kernel for flat scenes does without: its rounds are packets, and the extra
  // live registers would cost it the 8th wave per SIMD.
  constexpr bool CARRY = MODE != MODE_ABSORB_FLAT && (MODE != MODE_GENERAL_FLAT || VR_FLAT_ORDERED);
  __shared__ float wallS[VR_WALL_TABLE]; // (96 .. : the launch's scalar frame, vr_frame.hpp)
  // per-lane event counters live in LDS (fire-and-forget ds_add), not in 8 VGPRs.  (Five of them counted per WAVE in
  // scalar registers — 5 KB of LDS less, room for a 7th block per CU — was built and measured in round 3: slower at
  // 7 waves per SIMD and at 6; removed.)
  __shared__ unsigned cntS[8 * VR_BLOCK];
  __shared__ unsigned pqS[(VR_BLOCK / 64) * 128]; // packet query: per-wave frontier lists
  constexpr bool PQ_CACHE = (MODE == MODE_ABSORB_FLAT || MODE == MODE_GENERAL_FLAT) && (!RELIEF || VR_PQ_CACHE_RELIEF) && VR_PQ_CACHE != 0 && !PLANAR_LATTICE; // (pq_hit_packet CACHE: flat-scene kernels; the lattice kernel searches no tree)
  __shared__ float pqBoxS[PQ_CACHE ? (VR_BLOCK / 64) * 6 * VR_PQ_KEEP : 1];         // ... the kept leaf nodes' boxes, VR_PQ_KEEP x 6 per wave
  __shared__ uint4 candS[PQ_CREDIT ? (VR_BLOCK / 64) * VR_PQ_RECORDS : 1]; // ... and candidate records (pq_credit)
  // ... and, where the credits of a round carry different weights (the general kernels), one int64 sum per candidate
  // and data label (two labels here; further ones are summed over the wave in registers)
  constexpr bool PQ_SUMS = PQ_CREDIT && !ABSORB;
  constexpr unsigned PQ_LAB = EXT ? 2u : 1u;
  __shared__ unsigned long long candAccS[PQ_SUMS ? (VR_BLOCK / 64) * VR_PQ_CANDS * PQ_LAB : 1];
  // per-lane stack of the ordered walk, [entry][lane]; the absorbing flat-scene kernel walks rarely and keeps its
  // 8 waves per SIMD with a short LDS part (deeper entries: global slab)
  constexpr bool ORDERED = MODE != MODE_ABSORB_FLAT && (MODE != MODE_GENERAL_FLAT || VR_FLAT_ORDERED); // (MODE_ABSORB_FLAT walks rarely: it keeps the escape-link walk, one register of state)
  constexpr int SD = SMALL ? VR_SMALL_STACK : VR_STACK_LDS;
  __shared__ unsigned stackS[ORDERED ? SD * VR_BLOCK : 1];
  // (MODE 4: the scene copy is the kernel's dynamic LDS — smallBytes of it, so a smaller scene leaves room for a
  //  fifth block per CU)
  extern __shared__ uint4 sceneS[];
  unsigned char *const sceneB = reinterpret_cast<unsigned char *>(sceneS);
  const unsigned tid = threadIdx.x;
  // (the wave's index as a SCALAR: the per-wave tables' addresses are then wave-uniform values the compiler keeps in
  //  SGPRs — as per-lane values one of them was spilled and came back from scratch three times a round, each reload
  //  waiting for every atomic and load the wave had in flight)
  const unsigned waveInBlock = (unsigned)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
  cands.rec = (VR_LDS U4 *)(candS + (PQ_CREDIT ? waveInBlock * VR_PQ_RECORDS : 0u));
  const unsigned lane = tid & 63u;
  const unsigned gwave = (blockIdx.x * VR_BLOCK + tid) >> 6;
  if (tid < VR_WALL_TABLE)
    wallS[tid] = p.wallTable[tid];
  if (tid == VR_F_EXTRA_LO || tid == VR_F_EXTRA_HI) // (read per lane at a refill: as a kernel argument the pointer would be held in SGPRs throughout)
    wallS[tid] = __uint_as_float((unsigned)((unsigned long long)p.recExtra >> (tid == VR_F_EXTRA_LO ? 0 : 32)));
#pragma unroll
  for (int k = 0; k < 8; ++k)
    cntS[k * VR_BLOCK + tid] = 0u;
  if constexpr (PQ_CACHE) {
    if (tid < VR_BLOCK / 64)
      pqS[tid * 128 + 39] = 0u; // (no cached frontier yet: pq_hit_packet CACHE)
  }
  if (SMALL) {
    // stage the scene (the offsets are multiples of 16 bytes; vr_apply_prepare checked that it fits)
    const uint4 *gn = reinterpret_cast<const uint4 *>(p.pnodes);
    uint4 *ln = reinterpret_cast<uint4 *>(sceneB + p.smallOff[0]);
    for (unsigned k = tid; k < 2u * p.numNodes; k += VR_BLOCK)
      ln[k] = gn[k];
    const uint4 *gp = reinterpret_cast<const uint4 *>(p.prims);
    uint4 *lp = reinterpret_cast<uint4 *>(sceneB + p.smallOff[1]);
    for (unsigned k = tid; k < (GEO == 0 ? 2u : 4u) * p.numPrims; k += VR_BLOCK)
      lp[k] = gp[k];
    unsigned *lo = reinterpret_cast<unsigned *>(sceneB + p.smallOff[2]);
    for (unsigned k = tid; k <= p.numPrims; k += VR_BLOCK)
      lo[k] = p.nbOff[k];
    unsigned *li = reinterpret_cast<unsigned *>(sceneB + p.smallOff[3]);
    for (unsigned k = tid; k < p.smallNb; k += VR_BLOCK)
      li[k] = p.nbIds[k];
    unsigned long long *lf = reinterpret_cast<unsigned long long *>(sceneB + p.smallOff[4]);
    for (unsigned k = tid; k < p.numPrims * (p.numData + (STATS ? (unsigned)VR_STAT_PLANES : 0u)); k += VR_BLOCK) // (one plane per data label)
      lf[k] = 0ull;
    if (p.primSticking) {
      float *ls = reinterpret_cast<float *>(sceneB + p.smallOff[5]);
      for (unsigned k = tid; k < p.numPrims; k += VR_BLOCK)
        ls[k] = p.primSticking[k];
    }
  }
  __syncthreads();
  unsigned *const cnt = cntS + tid; // counter k of this lane: cnt[k * VR_BLOCK]
  enum { K_BOUNDARY = 0, K_REFL, K_TIER2, K_TRACES, K_NONGEO, K_GEO, K_TERM, K_PARTICLE };
#define VR_COUNT(k, v) atomicAdd(&cnt[(k)*VR_BLOCK], (unsigned)(v))

  // scene data: global memory, or (MODE 4) the block's LDS copies
  const float4 *__restrict__ prims = SMALL ? reinterpret_cast<const float4 *>(sceneB + p.smallOff[1])
                                           : reinterpret_cast<const float4 *>(p.prims);
  const uint4 *__restrict__ pnodes = SMALL ? reinterpret_cast<const uint4 *>(sceneB + p.smallOff[0])
                                           : reinterpret_cast<const uint4 *>(p.pnodes);
  const unsigned *__restrict__ nbOff = SMALL ? reinterpret_cast<const unsigned *>(sceneB + p.smallOff[2]) : p.nbOff;
  const unsigned *__restrict__ nbIds = SMALL ? reinterpret_cast<const unsigned *>(sceneB + p.smallOff[3]) : p.nbIds;
  const float *__restrict__ primSticking = SMALL ? reinterpret_cast<const float *>(sceneB + p.smallOff[5]) : p.primSticking;
  const float4 *__restrict__ rayAB = reinterpret_cast<const float4 *>(p.slotRec);
  unsigned long long *const fluxGlobal = p.fluxAcc + (size_t)(blockIdx.x & p.accMask) * p.accStride; // this block's replica
  unsigned long long *const fluxAcc = SMALL ? reinterpret_cast<unsigned long long *>(sceneB + p.smallOff[4]) : fluxGlobal;
  const float tnear = 1e-4f; // rayUtil.hpp:229-231

  // per-lane ray state
  bool active = false;
  // `dir` is what the intersector sees: the 2-D projection of rayDirection (rayUtil.hpp:204-227),
  // i.e. rayDirection itself in 3-D (then the same registers)
  V3 org = mk(0, 0, 0), rayDirection = mk(0, 0, 1), dir2 = mk(0, 0, 1);
  V3 &dir = D == 3 ? rayDirection : dir2;
  float rayWeight = 0.f;
  [[maybe_unused]] RayState rayState; // (SW > 0: the model's state, in registers from the ray's pick-up to its end)
  // The two per-ray counters are touched once per segment: in the general kernels they live in LDS, not in two of
  // the 80 VGPRs (left to the register allocator they went to scratch, and a scratch reload waits on the
  // vector-memory counter: for every load and atomic the wave has in flight).
  constexpr bool COLD_IN_LDS = !ABSORB && !SMALL;
  __shared__ unsigned coldS[COLD_IN_LDS ? 3 * VR_BLOCK : 1];
  unsigned numReflectionsR = 0, boundaryHitsR = 0;
  unsigned &numReflections = COLD_IN_LDS ? coldS[tid] : numReflectionsR;
  unsigned &boundaryHits = COLD_IN_LDS ? coldS[VR_BLOCK + tid] : boundaryHitsR;
  // Source::getInitialRayWeight(idx) (rayTraceKernel.hpp:124): 1 for every built-in source; a host-callback source may
  // hand over its own (p.hostWeights, wave-uniform test).  Read again only by the roulette's thresholds.
  unsigned initWeightR = 0x3F800000u;
  unsigned &initWeightBits = COLD_IN_LDS ? coldS[2 * VR_BLOCK + tid] : initWeightR;
  bool hitFromBack = false;
  bool start = false; // this lane begins a new trace segment in this round
  // (MODE 6) this wave's block of the spill queue: first record and records used (wave-uniform)
  unsigned spillBase = 0u, spillUsed = VR_SPILL_BLOCK;
  unsigned node = VR_END; // cursor of the lane's BVH walk (VR_END: none under way)
  unsigned sp = 0u;       // ... and the depth of its stack
  unsigned *const stackG = p.walkStack + (size_t)gwave * (VR_STACK_GLOBAL * 64u) + lane;
  HitRec h;               // closest hit so far of the lane's current segment
  h.t = 0.f;
  h.geom = -1;
  h.prim = 0u;
  h.pos = 0u;
  Rng rng;
  rng_resume(rng, 0u, 0u, 0ull, 0ull);
  rng.scratch = p.rngScratch + (size_t)gwave * (312u * 64u) + lane;
  // wave-uniform cursor over the sort bins: [curBin, spanEnd) is the span of (virtual)
  // bins this wave pulled from the queue; bins >= numBins are 64-ray chunks of the
  // overflow region
  typedef const unsigned __attribute__((address_space(4))) *ConstU32;
  ConstU32 binCount = (ConstU32)p.binCount;
  const unsigned ovCount = binCount[p.numBins] < p.ovCap ? binCount[p.numBins] : p.ovCap;
  const unsigned ovChunks = (ovCount + p.binCap - 1) / p.binCap;
  // (MODE 7: the spill queue's records, in chunks of a bin's capacity, are the virtual bins behind the overflow chunks)
  const unsigned spillN = (RESUME && p.spillRec) ? ((ConstU32)p.spillCount)[0] : 0u;
  // (the queue is made of 64-record blocks, each with a ray in its first record and possibly unused records at its end:
  //  a chunk of at least a block, block aligned, so that a refill which finds no ray has truly run out of work)
  const unsigned spillChunk = p.binCap < VR_SPILL_BLOCK ? VR_SPILL_BLOCK : (p.binCap / VR_SPILL_BLOCK) * VR_SPILL_BLOCK;
  const unsigned totalBins = p.numBins + ovChunks + (RESUME ? (spillN + spillChunk - 1) / spillChunk : 0u);
  unsigned curBin = 0, spanStart = 0, spanEnd = 0, curOff = 0, curCnt = 0, curBase = 0;
  unsigned spanCounts = 0; // lane i: ray count of bin spanStart + i
  // (only the general flat-scene kernel has the queues compiled in — it is the one they pay for, vr_apply.cpp — the others
  //  keep the single queue's code: MODE 1 with the bookkeeping: L2 hit rate 74 -> 84 % but 6.60 -> 6.83 ms from the
  //  extra scalar spills of a kernel at 8 waves per SIMD)
  constexpr bool MULTIQ = MODE == MODE_GENERAL_FLAT;
  const unsigned numQueues = MULTIQ ? p.numQueues : 1u;
  const unsigned myQueue = MULTIQ ? (blockIdx.x & (numQueues - 1u)) : 0u; // (numQueues is 1 or 8)
  unsigned qTried = 0;                      // queues this wave has found empty (wave-uniform)
  unsigned packetSkip = 0, packetFails = 0; // wave-uniform back-off of packet attempts
  unsigned pqSkip = 0, pqFails = 0;         // ... and of packet-query attempts
  bool exhausted = false;
  VR_DIAG_DECL
#ifdef VR_DIAG
  __shared__ unsigned long long phaseS[(VR_BLOCK / 64) * 16];
  unsigned long long *const phaseT = phaseS + (tid >> 6) * 16;
  if (lane < 16)
    phaseT[lane] = 0ull;
  unsigned long long tLast = __builtin_amdgcn_s_memtime();
#endif

  for (;;) {
    // keep the compiler from hoisting the (loop-invariant) LDS wall table into
    // ~100 registers: occupancy matters more than 24 ds_reads per segment
    asm volatile("" ::: "memory");
    // ---- wave-wide compaction / restart: idle lanes pull the next sorted rays ----
    // Two steps: first every idle lane is ASSIGNED a record slot — a wave-uniform walk over the next
    // bins of the span, no memory but the (rare) grab of a new span — then all of them load at once.
    // (Loading bin by bin cost one full HBM round trip per bin: a round of the absorbing kernel
    //  swallows two or three bins.)
    {
      const unsigned long long idle = ballot64(!active);
      const unsigned need = (unsigned)__popcll(idle);
      const unsigned rank = (unsigned)__popcll(idle & ((1ull << lane) - 1ull));
      unsigned slot = 0xFFFFFFFFu;
      unsigned assigned = 0;
      // (at most 12 bin changes per round — unless the wave has nothing at all to do: it owns its span, and
      //  leaving with bins of it unread would lose their rays)
      for (int adv = 0; assigned < need && (adv < 12 || (need == 64u && assigned == 0u));) {
        if (curOff >= curCnt) { // current bin used up: next bin of the span, or a new span
          ++adv;
          if (curBin + 1 >= spanEnd || spanEnd == 0) {
            if (exhausted)
              break;
            // ---- queue pull: a new span of bins from the work queue(s) ----
            // One queue of bins PER XCD: queue q owns the q-th eighth of the (spatially ordered) bins, the waves of
            // an XCD (blockIdx & 7 labels the blocks that share one) drain their own queue first and then help
            // with the others.  The rounds that follow each other on an XCD are then neighbours in space: the
            // primitive records one round pulled into the XCD's L2 serve the next (one global queue dealt
            // neighbouring spans to all eight L2s: 37 line misses per C2 round beyond its ray records).
            if constexpr (!MULTIQ) {
              unsigned long long s = 0;
              if (lane == 0)
                s = atomicAdd(p.workCounter, (unsigned long long)p.chunk);
              s = bcast64(s);
              if (s >= totalBins) {
                exhausted = true;
                break;
              }
              curBin = spanStart = (unsigned)s;
              spanEnd = (unsigned)((s + p.chunk < totalBins) ? s + p.chunk : totalBins);
            } else {
              unsigned lo = 0, hi = 0;
              for (; qTried < numQueues; ++qTried) {
                const unsigned q = (myQueue + qTried) & (numQueues - 1u);
                const unsigned qLo = (unsigned)((unsigned long long)totalBins * q / numQueues);
                const unsigned qHi = (unsigned)((unsigned long long)totalBins * (q + 1u) / numQueues);
                unsigned long long s = 0;
                if (lane == 0)
                  s = atomicAdd(p.workCounter + (size_t)q * VR_QUEUE_STRIDE, (unsigned long long)p.chunk);
                s = bcast64(s);
                if (s < (unsigned long long)(qHi - qLo)) {
                  lo = qLo + (unsigned)s;
                  hi = (lo + p.chunk < qHi) ? lo + p.chunk : qHi;
                  break;
                }
              }
              if (lo == hi) { // every queue is empty
                exhausted = true;
                break;
              }
              curBin = spanStart = lo;
              spanEnd = hi;
            }
            // the span's bin counts in one coalesced load (lane i <- bin spanStart + i; chunk <= 64)
            const unsigned bi = spanStart + lane;
            spanCounts = (bi < spanEnd && bi < p.numBins) ? p.binCount[bi] : 0u;
            // ---- (end of the queue pull: the bin walk goes on) ----
          } else {
            ++curBin;
          }
          curOff = 0;
          if (curBin < p.numBins) {
            const unsigned c = __shfl(spanCounts, (int)(curBin - spanStart), 64);
            curCnt = c < p.binCap ? c : p.binCap;
            curBase = curBin * p.binCap;
          } else if (!RESUME || curBin < p.numBins + ovChunks) {
            const unsigned k = (curBin - p.numBins) * p.binCap;
            curCnt = ovCount - k < p.binCap ? ovCount - k : p.binCap;
            curBase = p.numBins * p.binCap + k;
          } else { // a chunk of the spill queue: bit 31 marks its record numbers
            const unsigned k = (curBin - p.numBins - ovChunks) * spillChunk;
            curCnt = spillN - k < spillChunk ? spillN - k : spillChunk;
            curBase = 0x80000000u | k;
          }
          curCnt = __builtin_amdgcn_readfirstlane(curCnt);
          continue;
        }
        const unsigned avail = curCnt - curOff;
        const unsigned take = avail < need - assigned ? avail : need - assigned;
        if (!active && rank >= assigned && rank < assigned + take)
          slot = curBase + curOff + (rank - assigned);
        curOff += take;
        assigned += take;
      }
      bool resumed = false;
      if (RESUME && slot != 0xFFFFFFFFu && (slot >> 31)) {
        // a ray of the spill queue: its whole state as the relief kernel left it
        const float4 *__restrict__ sr = reinterpret_cast<const float4 *>(p.spillRec) + 4 * (size_t)(slot & 0x7FFFFFFFu);
        const float4 r0 = sr[0], r1 = sr[1], r2 = sr[2], r3 = sr[3];
        const bool ray = __float_as_uint(r2.w) != 0xFFFFFFFFu; // (the unused end of a wave's block: spill_pad)
        org = mk(r0.x, r0.y, r0.z);
        rayWeight = r0.w;
        rayDirection = mk(r1.x, r1.y, r1.z);
        dir = project_dir<D>(rayDirection);
        rng_resume(rng, __float_as_uint(r1.w), __float_as_uint(r2.x),
                   ((u64)__float_as_uint(r3.y) << 32) | __float_as_uint(r3.x), ((u64)__float_as_uint(r3.w) << 32) | __float_as_uint(r3.z));
        numReflections = __float_as_uint(r2.y);
        boundaryHits = __float_as_uint(r2.z) & 0x7FFFFFFFu;
        hitFromBack = (__float_as_uint(r2.z) >> 31) != 0u;
        active = ray;
        start = ray;
        resumed = true;
      }
      if (slot != 0xFFFFFFFFu && !resumed) {
        DIAG(8);
        const unsigned j = slot;
        const float4 a = rayAB[2 * (size_t)j]; // (32-byte records in both forms, vr_types.hpp)
        const float4 b = rayAB[2 * (size_t)j + 1];
        if (!ABSORB) {
          // compact form.  (The source frame comes from LDS, per lane: as kernel arguments these loop-invariant scalars
          //  were hoisted and held across the whole kernel — scalar spills in every instantiation.)
          float srcPlane = wallS[VR_F_SRC_PLANE];
          const int rd = __float_as_int(wallS[VR_F_RAYDIR]), fd = __float_as_int(wallS[VR_F_FIRSTDIR]);
          const unsigned long long ex = ((unsigned long long)__float_as_uint(wallS[VR_F_EXTRA_HI]) << 32) | __float_as_uint(wallS[VR_F_EXTRA_LO]);
          const unsigned seed32 = tea3((unsigned)(p.batchFirst + __float_as_uint(b.y)), p.seed);
          constexpr unsigned NS = D == 3 ? 4u : 3u; // draws of the plain generator (gen_kernel)
          unsigned k = NS;
          u64 lo;
          if (ex) { // a source with its own origin plane / draw count: the side array has them and s[k]
            typedef float F4 __attribute__((ext_vector_type(4)));
            const F4 e = reinterpret_cast<const __attribute__((address_space(1))) F4 *>(ex)[__float_as_uint(b.y)]; // (global, not flat)
            srcPlane = e.x;
            k = __float_as_uint(e.y);
            lo = ((u64)__float_as_uint(e.w) << 32) | __float_as_uint(e.z);
          } else {
            lo = seed32; // s[NS]: NS steps of the seeding recurrence
#pragma unroll
            for (unsigned st = 1; st <= NS; ++st)
              lo = mt_step(lo, st);
          }
          org.x = rd == 0 ? srcPlane : (fd == 0 ? a.x : a.y);
          org.y = rd == 1 ? srcPlane : (fd == 1 ? a.x : a.y);
          org.z = rd == 2 ? srcPlane : (fd == 2 ? a.x : a.y);
          rayDirection = mk(a.z, a.w, b.x);
          rng_resume(rng, seed32, k, lo, ((u64)__float_as_uint(b.w) << 32) | __float_as_uint(b.z));
        } else {
          org = mk(a.x, a.y, a.z);
          rayDirection = mk(a.w, b.x, b.y);
        }
        dir = project_dir<D>(rayDirection); // what Embree sees (rayUtil.hpp:204-227)
        rayWeight = 1.f;                    // Source::getInitialRayWeight
        if (!ABSORB && p.hostWeights) {     // (a host-callback source with weights of its own never runs an absorbing kernel)
          rayWeight = p.hostWeights[p.batchFirst + __float_as_uint(b.y)];
          initWeightBits = __float_as_uint(rayWeight);
        }
        if constexpr (SW > 0) { // what the model's init left (gen_state_kernel), indexed like the records' side array
          const float4 sv = reinterpret_cast<const float4 *>(frame_addr(wallS, VR_F_STATE_LO))[__float_as_uint(b.y)];
          rayState.v[0] = sv.x;
          rayState.v[1] = sv.y;
          rayState.v[2] = sv.z;
          rayState.v[3] = sv.w;
        }
        numReflections = 0;
        boundaryHits = 0;
        hitFromBack = false;
        active = true;
        start = true;
      }
    }
    // ---- round set-up: the exit vote, carried walks, the round's choice of search ----
    if (!ballot64(active))
      break;
    TICK(0);

    // ---- closest hit of a trace segment (rtcIntersect1, rayTraceKernel.hpp:163-167) ----
    // A round: if the whole wave begins a segment together
    // (freshly sorted, coherent rays) it first tries the wave-uniform packet traversal with
    // a bounded number of node visits; otherwise, and when the packet gives up, every lane
    // walks its own path — but only until the number of lanes still walking drops below
    // p.walkExit: the lanes that are done run the state machine and start their next
    // segment (or pull a new ray) while the stragglers keep their cursor and closest hit
    // for the next round, so one long walk does not idle the other 63 lanes.
    if (active) {
      DIAG(0);
    }
    if (start) {
      DIAG(9);
    }
    if (!CARRY || start) { // (!CARRY: every active lane starts a segment in every round)
      hit_clear(h);
      node = 0u;
    }
    const unsigned long long carried = CARRY ? ballot64(active && !start) : 0ull;
    start = false;
    const bool usePacket = !SMALL &&
        !(p.debugFlags & 32u) && carried == 0ull && packetSkip == 0 && __popcll(ballot64(active)) >= 8;
    bool packetDone = false;
    bool pqCredit = false; // this round's surface hits are credited from the packet's candidate list
    [[maybe_unused]] bool wallFree = false; // PLANAR_ROUND: no active lane of this round can meet a wall before its plane hit (wave-uniform)
    if (!SMALL && usePacket && p.wide && !(p.debugFlags & 128u)) {
      // first choice: the box query (one wide-tree search for the whole wave)
      if (pqSkip == 0) {
        if (active) {
          DIAG(12);
        }
        // ---- walls first ----
        // (the walls first for the flat-scene kernels' queries: see pq_hit_packet, tWall.  The conservative pre-tests of
        //  hit_walls let only the rays near a side wall through to the exact test)
        float tWall = 3.402823466e+38f;
        if constexpr (PLANAR_ROUND) {
          // the round's point (vr_planar_disks.hpp (1)), and the vote on its walls (3): where every active lane starts
          // inside the walls and lands well inside them, no wall can come before a plane hit — no wall test before the
          // query (tWall stays infinite), and behind it only for the lanes the query left without a hit
          const int pa = __float_as_int(wallS[VR_F_PD_AXIS]);
          const float s = wallS[VR_F_UD_N + pa];
          cands.round = planar_round_point(active, org.x, org.y, org.z, dir.x, dir.y, dir.z, getc(org, pa), getc(dir, pa) * s, tnear,
                                           wallS[VR_F_PD_COORD], s, wallS[VR_F_UD_RADIUS], wallS[VR_F_UD_T]);
          const int a1 = __float_as_int(wallS[VR_F_FIRSTDIR]), a2 = __float_as_int(wallS[VR_F_SECONDDIR]);
          const V3 q = mk(cands.round.qx, cands.round.qy, cands.round.qz);
          const PlanarWallRect wr{wallS[VR_F_LO1], wallS[VR_F_LO1 + 1], wallS[VR_F_LO1 + 2], wallS[VR_F_LO1 + 3]};
          const PlanarWallRect wi{wallS[VR_F_PR_IN], wallS[VR_F_PR_IN + 1], wallS[VR_F_PR_IN + 2], wallS[VR_F_PR_IN + 3]};
          const bool walled = active && !planar_wall_free(getc(org, a1), getc(org, a2), getc(q, a1), getc(q, a2), wr, wi);
          wallFree = ballot64(walled) == 0ull;
        }
        if constexpr ((MODE == MODE_ABSORB_FLAT || MODE == MODE_GENERAL_FLAT) && VR_PQ_WALLS_FIRST) {
          if (active && !wallFree && !(p.debugFlags & 65536u)) { // (flag 65536: off, for comparison)
            HitRec hw;
            hit_clear(hw);
            if constexpr (FRAME_LDS)
              hit_walls_lds(p, wallS, org, dir, tnear, hw);
            else
              hit_walls(p, wallS, org, dir, tnear, hw);
            tWall = hw.geom == 0 ? hw.t : tWall;
          }
        }
        // ---- packet query: the call and its back-off ----
        if constexpr (LATTICE_LANES) // (... and four disk tests per lane in place of the candidate loop)
          packetDone = pq_hit_lattice_lanes<PQ_CREDIT>(p, h, cands, wallS, tWall VR_DIAG_PASS);
        else if constexpr (PLANAR_LATTICE) // (the lattice table's window in place of the search: no frontier lists, no leaf-node boxes)
          packetDone = pq_hit_lattice<PQ_CREDIT>(p, h, cands, wallS, tWall VR_DIAG_PASS);
        else
          packetDone = pq_hit_packet<GEO, PQ_CREDIT, FRAME_LDS, FOLLOW, RELIEF, PQ_CACHE, LEAN, UNIFORM, PLANAR, PLANAR_ROUND>(p, active, org, dir, tnear, h, (volatile VR_LDS unsigned *)(pqS + waveInBlock * 128u), cands, wallS, (volatile VR_LDS float *)(pqBoxS + (PQ_CACHE ? waveInBlock * (6u * VR_PQ_KEEP) : 0u)), tWall VR_DIAG_PASS);
        pqCredit = PQ_CREDIT && packetDone;
        pqFails = packetDone ? 0u : (pqFails < 6u ? pqFails + 1u : 6u);
        pqSkip = packetDone ? 0u : (1u << pqFails) - 1u;
        if (packetDone) {
          node = VR_END;
          if (active) {
            DIAG(13);
          }
        }
      } else {
        --pqSkip;
      }
    }
    // ---- fall-back: the packet traversal, then the per-lane walk ----
    if (!SMALL && usePacket && !packetDone) {
      packetDone = bvh_hit_packet<GEO>(p, active, org, dir, tnear, h, p.packetBudget, p.packetRatio VR_DIAG_PASS);
      // a wave whose rays have scattered stops paying for hopeless packets for a while
      packetFails = packetDone ? 0u : (packetFails < 6u ? packetFails + 1u : 6u);
      packetSkip = packetDone ? 0u : (1u << packetFails) - 1u;
      if (packetDone)
        node = VR_END;
    } else if (packetSkip) {
      --packetSkip;
    }
    TICK(1);
    if (!packetDone) {
      const unsigned walking = (unsigned)__popcll(ballot64(active && (ORDERED ? node != VR_END : node < p.numNodes)));
      const unsigned minLanes = (!CARRY || exhausted || walking <= p.walkExit) ? 1u : p.walkExit;
      if (ORDERED)
        pair_walk_lanes<GEO, SD, MODE != MODE_ABSORB>(p, pnodes, prims, stackS + tid, stackG, active, org, dir, tnear, h, node, sp, minLanes VR_DIAG_PASS);
      else
        bvh_walk_lanes<GEO>(p, active, org, dir, tnear, h, node, minLanes VR_DIAG_PASS);
    }
    const bool fin = active && (ORDERED ? node == VR_END : node >= p.numNodes); // this lane's geometry walk is complete
#ifdef VR_SELFCHECK
    { // -DVR_SELFCHECK build: every finished segment again with the escape-link walk; disagreements are
      // counted in counters[C_CHECK], the first one is kept in counters[C_CHECK_RAY..]
      HitRec hb;
      hit_clear(hb);
      unsigned nb = fin ? 0u : VR_END;
      bvh_walk_lanes<GEO>(p, fin, org, dir, tnear, hb, nb, 1u VR_DIAG_PASS);
      // (the CLOSEST HIT is what is compared — geometry and walls: a packet query leaves a ray that meets a side wall before
      //  it can enter the scene box without a geometry hit, and the wall wins either way)
      HitRec hc = h;
      if (fin) {
        hit_walls(p, wallS, org, dir, tnear, hb);
        hit_walls(p, wallS, org, dir, tnear, hc);
      }
      if (fin && (hb.geom != hc.geom || hb.t != hc.t || (hb.geom == 1 && hb.pos != hc.pos) || (hb.geom == 0 && hb.prim != hc.prim))) {
        if (atomicAdd(&p.counters[C_CHECK], 1ull) == 0ull) {
          const float v[8] = {org.x, org.y, org.z, dir.x, dir.y, dir.z, hc.t, hb.t};
          for (int k = 0; k < 8; ++k)
            p.counters[C_CHECK_RAY + k] = (unsigned long long)__float_as_uint(v[k]);
          p.counters[C_CHECK_POS] = ((unsigned long long)hc.pos << 32) | hb.pos;
          p.counters[C_CHECK_GEOM] = ((unsigned long long)(unsigned)hc.geom << 32) | (unsigned)hb.geom;
        }
      }
    }
#endif
    TICK(3);
    // ---- walls of the finished segments ----
    if (fin && !(PLANAR_ROUND && wallFree && h.geom >= 0)) { // boundary walls, where one can come before the hit
      if constexpr (FRAME_LDS)
        hit_walls_lds(p, wallS, org, dir, tnear, h);
      else
        hit_walls(p, wallS, org, dir, tnear, h);
    }
    TICK(4);
    // ---- the aggregation vote, then the state machine ----
    // Merge same-disk credits of the wave into one atomic when that is likely to pay: rays of a
    // packet, or — sampled on one lane's target — when a good share of the wave's hits fall on
    // the same primitive (sorted rays on a coarse scene: one vector atomic with 64 lanes on ONE
    // address is serialised lane by lane in the L2 atomic unit).
    bool aggregate = packetDone || (p.debugFlags & 32768u) != 0u; // (flag 32768: always, a measurement)
    {
      const bool cand = fin && h.geom == 1;
      const unsigned long long cm = ballot64(cand);
      if (!aggregate && cm) {
        const unsigned sample = (unsigned)__shfl((int)h.pos, __ffsll((long long)cm) - 1, 64);
        const unsigned same = (unsigned)__popcll(ballot64(cand && h.pos == sample));
        aggregate = 4u * same >= (unsigned)__popcll(cm) && same >= 4u;
      }
    }

    bool creditLane = false;
    u64 creditW = 0;
    float creditWf = 0.f; // (registry particles: the weight as the model's collide sees it ...
    V3 creditDir = mk(0.f, 0.f, 0.f); //  ... and the INCOMING direction: the state machine replaces it by the reflected one)
    SUB_MARK(12); // (since the walls: the aggregation vote)
    if (fin) {
      DIAG(5);
      // ---- the reference's state machine for this segment (rayTraceKernel.hpp:169-335) ----
      VR_COUNT(K_TRACES, 1);
      if (h.geom < 0) { // miss, :172-176
        VR_COUNT(K_NONGEO, 1);
        active = false;
      } else {
        const V3 hitPoint = mk(org.x + dir.x * h.t, org.y + dir.y * h.t, org.z + dir.z * h.t);
        bool scattered = false;
        if (EXT && EXT_FULL && p.meanFreePath > 0.f) {
          // mean-free-path scatter (rayTraceKernel.hpp:179-203), quirk Q1 kept: tested after the
          // closest hit was found, and the origin moves by dir * rnd (the uniform number itself)
          const float rnd = canon_f32(rng_next(rng, cnt[K_TIER2 * VR_BLOCK]));
          const float scatterProbability = (float)(1. - (double)glibc_expf(-h.t / p.meanFreePath));
          if (rnd < scatterProbability) {
            org = mk(org.x + dir.x * rnd, org.y + dir.y * rnd, org.z + dir.z * rnd);
            rayDirection = pick_random_point_on_unit_sphere(rng, cnt[K_TIER2 * VR_BLOCK]);
            dir = project_dir<D>(rayDirection);
            VR_COUNT(K_PARTICLE, 1);
            scattered = true;
          }
        }
        if (scattered) {
          // (reflect = true; continue)
        } else if (h.geom == 0) { // boundary, :206-214 + rayBoundary.hpp:29-127
          SUB_START
          if (++boundaryHits > p.maxBoundaryHits) {
            VR_COUNT(K_TERM, 1);
            active = false;
          } else {
            process_boundary_hit<D>(p, wallS, h.prim, hitPoint, org, rayDirection, dir, active);
          }
          SUB_STOP(11);
        } else {
          // geometry hit
          V3 geomNormal;
          if (GEO == 0) {
            if (LATTICE_LANES && pqCredit) {
              // (uniform disks: every record's normal is record 0's word for word — uniform_disks_kernel compares the
              //  words — and the frame's VR_F_UD_N are those words: the bits the record would give)
              geomNormal = mk(wallS[VR_F_UD_N], wallS[VR_F_UD_N + 1], wallS[VR_F_UD_N + 2]);
            } else if (PQ_CREDIT && pqCredit) { // (found by the packet query: the candidate's record in LDS, not a dependent global load)
              const U4 nr = cands.rec[VR_PQ_NRM + cands.mine];
              geomNormal = mk(__uint_as_float(nr.x), __uint_as_float(nr.y), __uint_as_float(nr.z));
            } else {
              const float4 n4 = prims[2 * h.pos + 1];
              geomNormal = mk(n4.x, n4.y, n4.z);
            }
          } else {
            geomNormal = mk(prims[4 * h.pos + 1].w, prims[4 * h.pos + 2].w, prims[4 * h.pos + 3].w);
          }
          const bool backfaceHit = vdot(rayDirection, geomNormal) > 0.f; // :224
          SUB_MARK(10);
          if (backfaceHit) {
            if (GEO == 0 && !hitFromBack) { // first back hit of a disk: let through, :235-240
              hitFromBack = true;
              org = hitPoint;
            } else { // :229-233, :243-248
              VR_COUNT(K_TERM, 1);
              active = false;
            }
          } else {
            VR_COUNT(K_GEO, 1);
            DIAG(11);
            const u64 wfx = weight_fx(rayWeight);
            if (PQ_CREDIT && pqCredit) {
              creditLane = true; // credited after the state machine, for the whole wave at once (pq_credit)
              creditW = wfx;
              creditWf = rayWeight;
              if (EXT)
                creditDir = rayDirection;
            } else if (!EXT) {
              // surfaceCollision, rayParticle.hpp:148-156.  Without aggregation the credits of the neighbour
              // disks are first collected (three in registers; further ones, rare, go out at once) and then issued
              // together with the closest disk's: on gfx9 a load that follows an atomic waits for that atomic too
              // (one in-order counter), so an atomic inside the neighbour loop exposed its full L2 round trip to
              // the next neighbour's loads, iteration after iteration.
              unsigned cq0 = 0xFFFFFFFFu, cq1 = 0xFFFFFFFFu, cq2 = 0xFFFFFFFFu;
              if (aggregate && !(p.debugFlags & 1u))
                credit_aggregated(fluxAcc, true, h.pos, wfx);
              if (GEO == 0 && !(p.debugFlags & 4u)) {
                // every overlapping neighbour disk is credited the full weight (:271-300)
                SUB_START
                const unsigned nb = nbOff[h.pos], ne = nbOff[h.pos + 1];
                // One dependent access per neighbour instead of three: the next id is fetched while this
                // neighbour is tested, and both record words are requested together (left to itself the compiler
                // sinks the centre's load behind the normal's sign test).  Throughput of full launches does not
                // notice; a launch of 10^6 rays is as long as its longest bounce chain, and this loop was
                // half of a round's chain of memory latencies.
                unsigned qNext = nb < ne ? nbIds[nb] : 0u;
                for (unsigned j = nb; j < ne; ++j) {
                  DIAG(6);
                  const unsigned q = qNext;
                  qNext = nbIds[j + 1 < ne ? j + 1 : j];
                  const float4 c4 = prims[2 * q];
                  const float4 n4 = prims[2 * q + 1];
                  asm volatile("" ::"v"(c4.x), "v"(n4.x)); // (both in flight before the test branches)
                  const bool hitN = local_disc_hit(org, dir, c4, mk(n4.x, n4.y, n4.z)) && !(p.debugFlags & 1u);
                  if (aggregate) {
                    credit_aggregated(fluxAcc, hitN, q, wfx);
                  } else if (hitN) {
                    if (cq2 != 0xFFFFFFFFu)
                      atomicAdd(&fluxAcc[q], wfx);
                    else if (cq1 != 0xFFFFFFFFu)
                      cq2 = q;
                    else if (cq0 != 0xFFFFFFFFu)
                      cq1 = q;
                    else
                      cq0 = q;
                  }
                }
                SUB_STOP(8);
              }
              if (!aggregate && !(p.debugFlags & 1u)) {
                atomicAdd(&fluxAcc[h.pos], wfx);
                if (cq0 != 0xFFFFFFFFu)
                  atomicAdd(&fluxAcc[cq0], wfx);
                if (cq1 != 0xFFFFFFFFu)
                  atomicAdd(&fluxAcc[cq1], wfx);
                if (cq2 != 0xFFFFFFFFu)
                  atomicAdd(&fluxAcc[cq2], wfx);
              }
            } else {
              // plug-in particles: Particles::collide decides what each credited primitive's data
              // labels receive; with WDIST the weight is shared by inverse impact distance
              // (rayTraceKernel.hpp:258-296: w / d_i / sum(1/d) * numDisksHit, closest disk first)
              const int kind = p.particleKind;
              const ModelCtx mctx = model_ctx(p);
              // (a coarse scene under sorted rays: a good share of the wave credits ONE disk — merged per distinct
              //  weight like the built-in particles' credits, or the 64 lanes queue up on one address in L2)
              // (flux statistics: label 0's two companions, through the same path as the credit itself)
              [[maybe_unused]] auto creditStats = [&](unsigned q, float v) {
                unsigned long long *sq = fluxAcc + (size_t)p.numData * (SMALL ? p.numPrims : p.planeStride);
                unsigned long long *hits = sq + (SMALL ? p.numPrims : p.planeStride);
                if (aggregate && !SMALL) {
                  credit_aggregated(sq, true, q, weight_sq_fx(v));
                  credit_aggregated(hits, true, q, 1ull);
                } else {
                  atomicAdd(&sq[q], weight_sq_fx(v));
                  atomicAdd(&hits[q], 1ull);
                }
              };
              auto creditTo = [&](unsigned q, float w, const V3 &nq, unsigned origId) {
                if constexpr (SW > 0) { // (a stateful model: the ray's state and the primitive's material id too)
                  Particles::collide<EXT_FULL>(kind, mctx, rayState, w, rayDirection, nq, origId, material_of(wallS, origId),
                                               [&](int label, float v) {
                                                 unsigned long long *plane = fluxAcc + (size_t)label * (SMALL ? p.numPrims : p.planeStride);
                                                 if (aggregate && !SMALL)
                                                   credit_aggregated(plane, true, q, weight_fx(v));
                                                 else
                                                   atomicAdd(&plane[q], weight_fx(v));
                                                 if constexpr (STATS) {
                                                   if (label == 0)
                                                     creditStats(q, v);
                                                 }
                                               });
                } else {
                  Particles::collide<EXT_FULL>(kind, mctx, w, rayDirection, nq, origId, [&](int label, float v) {
                    unsigned long long *plane = fluxAcc + (size_t)label * (SMALL ? p.numPrims : p.planeStride);
                    if (aggregate && !SMALL) // (LDS accumulators take 64 adds on one address in their stride)
                      credit_aggregated(plane, true, q, weight_fx(v));
                    else
                      atomicAdd(&plane[q], weight_fx(v));
                    if constexpr (STATS) {
                      if (label == 0)
                        creditStats(q, v);
                    }
                  });
                }
              };
              if (GEO == 0) {
                const unsigned nb = nbOff[h.pos], ne = nbOff[h.pos + 1];
                float invSum = 0.f, dClosest = 0.f;
                unsigned numHit = 1;
                if (EXT_FULL && p.useWdist) {
                  const float4 cp = prims[2 * h.pos];
                  const V3 dv = mk(hitPoint.x - cp.x, hitPoint.y - cp.y, hitPoint.z - cp.z);
                  dClosest = sqrtf(vdot(dv, dv)) + 1e-6f;
                  invSum = 0.f + 1.f / dClosest;
                  for (unsigned j = nb; j < ne; ++j) {
                    const unsigned q = nbIds[j];
                    const float4 n4 = prims[2 * q + 1];
                    float dist;
                    if (local_disc_hit_dist(org, dir, prims[2 * q], mk(n4.x, n4.y, n4.z), dist)) {
                      invSum += 1.f / (dist + 1e-6f);
                      ++numHit;
                    }
                  }
                }
                creditTo(h.pos, (EXT_FULL && p.useWdist) ? rayWeight / dClosest / invSum * (float)numHit : rayWeight, geomNormal, h.prim);
                // (as in the built-in particles' loop: the next id is fetched while this neighbour is tested, and both
                //  record words are requested together — one dependent access per neighbour instead of three)
                unsigned qNext = nb < ne ? nbIds[nb] : 0u;
                for (unsigned j = nb; j < ne; ++j) {
                  const unsigned q = qNext;
                  qNext = nbIds[j + 1 < ne ? j + 1 : j];
                  const float4 c4 = prims[2 * q];
                  const float4 n4 = prims[2 * q + 1];
                  asm volatile("" ::"v"(c4.x), "v"(n4.x));
                  const V3 nq = mk(n4.x, n4.y, n4.z);
                  float dist;
                  if (local_disc_hit_dist(org, dir, c4, nq, dist))
                    creditTo(q, (EXT_FULL && p.useWdist) ? rayWeight / (dist + 1e-6f) / invSum * (float)numHit : rayWeight, nq,
                             __float_as_uint(n4.w));
                }
              } else {
                creditTo(h.pos, rayWeight, geomNormal, h.prim);
              }
            }
            if (ABSORB) {
              // sticking >= 1: weight drops to <= 0 (:316-319); the reflection draws
              // the reference makes before that test (Q2) are not observable.
              active = false;
            } else {
              // (not `p.primSticking ? primSticking[h.pos] : p.sticking`: the compiler makes that ONE load from a selected
              //  address — a generic pointer, i.e. a flat_load per reflection that waits on both memory counters)
              float sticking = p.sticking;
              asm volatile("" : "+s"(sticking)); // (a value in a register, not a second address to choose from)
              if (p.primSticking)
                sticking = primSticking[h.pos];
              [[maybe_unused]] V3 stateDir;
              if constexpr (SW > 0) {
                // a stateful model: ONE surfaceReflection call gives the sticking and the new direction and may update
                // the state (rayTraceKernel.hpp:310) — also for a ray it kills: draws after its end are not observable
                const Reflection r = Particles::surface_reflection<D, EXT_FULL>(
                    p.particleKind, model_ctx(p), rayState, rayWeight, rayDirection, geomNormal, h.prim,
                    material_of(wallS, h.prim), sticking, rng, cnt[K_TIER2 * VR_BLOCK]);
                sticking = r.sticking;
                stateDir = r.dir;
              } else if (EXT) { // (a registry model may make it depend on the primitive and the caller's global data)
                sticking = Particles::sticking<EXT_FULL>(p.particleKind, model_ctx(p), h.prim, sticking);
              }
              const float wAfter = rayWeight - rayWeight * sticking;
              if (wAfter <= 0.f) {
                active = false; // as above: the pending draws die with the ray
              } else {
                // surfaceReflection, rayParticle.hpp:137-146 / 178-187
                SUB_START
                V3 newDir;
                if constexpr (SW > 0)
                  newDir = stateDir;
                else if (PARTICLE == 0)
                  newDir = reflection_diffuse<D>(geomNormal, rng, cnt[K_TIER2 * VR_BLOCK]);
                else if (PARTICLE == 1)
                  newDir = reflect_specular(rayDirection, geomNormal);
                else
                  newDir = Particles::reflect<D, EXT_FULL>(p.particleKind, model_ctx(p), rayDirection, geomNormal, rng, cnt[K_TIER2 * VR_BLOCK]);
                rayWeight = wAfter;
                if (++numReflections > p.maxReflections) { // :320-324
                  VR_COUNT(K_TERM, 1);
                  active = false;
                } else {
                  // rejectionControl, :435-460
                  const float initWeight = p.hostWeights ? __uint_as_float(initWeightBits) : 1.f;
                  const float lowerThreshold = (float)(0.1 * (double)initWeight);
                  const float renewWeight = (float)(0.3 * (double)initWeight);
                  bool reflect = true;
                  if (!(rayWeight >= lowerThreshold)) {
                    DIAG(10);
                    const double killProbability = 1.0 - (double)(rayWeight / renewWeight);
                    if (canon_f64(rng_next(rng, cnt[K_TIER2 * VR_BLOCK])) < killProbability)
                      reflect = false;
                    else
                      rayWeight = renewWeight;
                  }
                  if (!reflect) {
                    active = false;
                  } else {
                    rayDirection = newDir;
                    org = hitPoint;
                    dir = project_dir<D>(rayDirection);
                  }
                }
                SUB_STOP(9);
              }
            }
          }
        }
      }
      SUB_MARK(13); // (since the walls: everything but the per-ray end counters)
      if (!active) {
        VR_COUNT(K_BOUNDARY, boundaryHits);
        VR_COUNT(K_REFL, numReflections);
      }
      start = active; // still alive: the next segment begins in the next round
    }
    TICK(5);
    // ---- crediting of a packet-query round ----
    if (PQ_CREDIT && pqCredit && !(p.debugFlags & 1u)) {
      // ---- surfaceCollision for the round's surface hits, candidate by candidate (wave-uniform):
      // a lane credits candidate q if q is its closest disk, or q is a neighbour of that disk
      // (centres within nbDist: the relation the CSR was built from, rayPointNeighborhood.hpp:287-298,
      // evaluated on the same floats) and its ray passes the neighbour test on q.  All lanes
      // crediting q add to ONE address: a single atomic (absorbing: count x unit weight).
      if (ballot64(creditLane)) {
        // centre of this lane's closest disk (LATTICE_LANES: cands.mine is one of the lane's four corners, its record in that corner's slot)
        const U4 own = cands.rec[!creditLane ? 0u : LATTICE_LANES ? (cands.slots >> (8u * cands.mine)) & 0xFFu : cands.mine];
        const float px = __uint_as_float(own.y), py = __uint_as_float(own.z), pz = __uint_as_float(own.w);
        const float dist = p.nbDist, dist2 = dist * dist;
        // General kernels: the lanes crediting candidate c add their fixed-point weights to the wave's LDS sum of c
        // (ds_add_u64: exact, any order) and afterwards lane c sends candidate c's total to HBM — ONE wave instruction
        // of global atomics per round and label instead of one atomic per candidate and distinct weight.
        // (from the per-lane wave index: with a wave-uniform ADDRESS the compiler turns these LDS atomics into a reduction
        //  over the wave plus one atomic — more work than the two or three lanes that credit a candidate; C2 0.1 +19 %)
        unsigned long long *const candAcc = candAccS + (PQ_SUMS ? (tid >> 6) * (VR_PQ_CANDS * PQ_LAB) : 0u);
        if (PQ_SUMS) {
          for (unsigned k = lane; k < cands.count * PQ_LAB; k += 64u)
            candAcc[k] = 0ull;
          __builtin_amdgcn_wave_barrier();
        }
        if constexpr (LATTICE_LANES) {
          // Four corners per lane (pq_hit_lattice_lanes): the `sel` rule of the loop below on each of the lane's own four
          // disks — the same expression on the same centre bits — and every selected disk's count goes up by one in the
          // wave's LDS counters, slot by slot (ds_add_u32 without return; integer adds, any order).  Then, as below, lane l
          // sends slot l's count in ONE wave instruction of atomics on distinct addresses: a slot is a lattice cell, its
          // disk no other slot's.
          if (cands.count != 0u) {
            // A round of the DIRECT form (the window did not fit the wave; wave-uniform): record l holds lane l's four leaf
            // positions, not a window.  The kernel's per-lane path for unpacketed hits, on the four corners: the closest
            // disk, and every corner that is its neighbour (the `near` relation of the CSR, on the same centre bits, read
            // from the records) and passes the neighbour test, each through credit_aggregated.  Integer sums: the fall-back's.
            const U4 pp = cands.rec[lane];
            const unsigned ps[4] = {pp.x, pp.y, pp.z, pp.w};
            const float4 oc = prims[2 * (size_t)(creditLane ? h.pos : 0u)];
#pragma unroll
            for (unsigned k = 0; k < 4u; ++k) {
              DIAG(6);
              const bool there = ps[k] != VR_LATTICE_EMPTY;
              const float4 c4 = prims[2 * (size_t)(there ? ps[k] : 0u)];
              const float dx = oc.x - c4.x, dy = oc.y - c4.y, dz = oc.z - c4.z;
              const float ax = fabsf(dx), ay = fabsf(dy), az = fabsf(dz);
              const bool near = (ax <= dist) & (ay <= dist) & ((p.geoD == 2) | (az <= dist)) & (((dx * dx + dy * dy) + dz * dz) <= dist2);
              const bool sel = creditLane & there & ((h.pos == ps[k]) | (near & (((cands.local >> k) & 1ull) != 0ull)));
              credit_aggregated(fluxAcc, sel, ps[k], 1099511627776ull);
            }
          } else {
          VR_LDS unsigned *const cntL = (VR_LDS unsigned *)(cands.rec + VR_PQ_LANE_CNT);
          cntL[lane] = 0u;
          __builtin_amdgcn_wave_barrier();
          // (corner by corner, read, test, add.  The four records read together first and the adds behind them — one trip
          //  to LDS in place of four — was built and measured: trace 2.43 ms against 2.38 ms this way, twice.)
#pragma unroll
          for (unsigned k = 0; k < 4u; ++k) {
            DIAG(6);
            const unsigned s = (cands.slots >> (8u * k)) & 0xFFu;
            const bool there = s != VR_PQ_NO_SLOT;
            const unsigned sl = there ? s : 0u;
            const U4 cr = cands.rec[sl];
            const float dx = px - __uint_as_float(cr.y), dy = py - __uint_as_float(cr.z), dz = pz - __uint_as_float(cr.w);
            const float ax = fabsf(dx), ay = fabsf(dy), az = fabsf(dz);
            const bool near = (ax <= dist) & (ay <= dist) & ((p.geoD == 2) | (az <= dist)) & (((dx * dx + dy * dy) + dz * dz) <= dist2);
            const bool sel = creditLane & there & ((h.pos == cr.x) | (near & (((cands.local >> k) & 1ull) != 0ull)));
            if (sel)
              __hip_atomic_fetch_add(cntL + sl, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
          }
          __builtin_amdgcn_wave_barrier();
          const unsigned mine = cntL[lane];
          if (mine)
            atomicAdd(&fluxAcc[cands.rec[lane].x], (u64)mine * 1099511627776ull); // unit weights: count x 2^40
          }
        } else if constexpr (LEAN) {
          // The absorbing flat-scene kernel: unit weights, so candidate c receives (lanes crediting it) x 2^40.  The vote
          // per candidate leaves its count with LANE c, and the lanes then send all the counts in ONE wave instruction of
          // atomics on distinct addresses.  (One single-lane atomic per candidate — behind a branch on the vote, a
          // first-lane election and the scalar address of fluxAcc[q] — was 36 scalar instructions per candidate, a
          // quarter of the scalar work of a round: profiles/salu_inventory_mode1.md.  Integer adds: the sums are the same.)
          unsigned mine = 0u; // lane c: the number of lanes that credit candidate c (cands.count <= VR_PQ_CANDS < 64)
          for (unsigned c = 0; c < cands.count; ++c) {
            DIAG(6);
            const U4 cr = cands.rec[c];
            const float dx = px - __uint_as_float(cr.y), dy = py - __uint_as_float(cr.z), dz = pz - __uint_as_float(cr.w);
            // (every condition evaluated, combined at the end: no divergent branch)
            const float ax = fabsf(dx), ay = fabsf(dy), az = fabsf(dz);
            const bool near = (ax <= dist) & (ay <= dist) & ((p.geoD == 2) | (az <= dist)) & (((dx * dx + dy * dy) + dz * dz) <= dist2);
            const bool sel = creditLane & ((h.pos == cr.x) | (near & (((cands.local >> c) & 1ull) != 0ull)));
            const unsigned n = (unsigned)__popcll(ballot64(sel));
            mine = lane == c ? n : mine;
          }
          if (lane < cands.count && mine)
            atomicAdd(&fluxAcc[cands.rec[lane].x], (u64)mine * 1099511627776ull); // unit weights: count x 2^40
        } else
        for (unsigned c = 0; c < cands.count; ++c) {
          DIAG(6);
          const U4 cr = cands.rec[c];
          const unsigned q = (unsigned)__builtin_amdgcn_readfirstlane((int)cr.x);
          const float dx = px - __uint_as_float(cr.y), dy = py - __uint_as_float(cr.z), dz = pz - __uint_as_float(cr.w);
          bool near = fabsf(dx) <= dist && fabsf(dy) <= dist && (p.geoD == 2 || fabsf(dz) <= dist);
          near = near && ((dx * dx + dy * dy) + dz * dz) <= dist2;
          const bool sel = creditLane && (h.pos == q || (near && ((cands.local >> c) & 1ull)));
          if (EXT) {
            // registry particles: the model's collide runs per lane with candidate q's own normal and id; its credits
            // are RECORDED per lane (a model may credit under any condition of its own) and then added label by label
            if (ballot64(sel)) {
              const float4 n4 = prims[2 * (size_t)q + 1];
              float val[VR_MAX_LABELS];
#pragma unroll
              for (int l = 0; l < VR_MAX_LABELS; ++l)
                val[l] = 0.f;
              [[maybe_unused]] u64 statSq = 0ull, statHits = 0ull; // (flux statistics: this lane's credits to label 0 of q)
              if (sel)
                Particles::collide<EXT_FULL>(p.particleKind, model_ctx(p), creditWf, creditDir, mk(n4.x, n4.y, n4.z),
                                             __float_as_uint(n4.w), [&](int label, float v) {
#pragma unroll
                                               for (int l = 0; l < VR_MAX_LABELS; ++l)
                                                 val[l] = l == label ? val[l] + v : val[l];
                                               if constexpr (STATS) {
                                                 if (label == 0) {
                                                   statSq += weight_sq_fx(v);
                                                   statHits += 1ull;
                                                 }
                                               }
                                             });
              if constexpr (STATS) { // (one integer wave sum and one atomic per plane, like the labels beyond the LDS sums)
                credit_wave_sum(fluxAcc + (size_t)p.numData * p.planeStride, q, statSq);
                credit_wave_sum(fluxAcc + (size_t)(p.numData + 1u) * p.planeStride, q, statHits);
              }
#pragma unroll
              for (int l = 0; l < VR_MAX_LABELS; ++l) {
                if ((unsigned)l >= p.numData)
                  break;
                if ((unsigned)l < PQ_LAB) {
                  if (sel)
                    atomicAdd(&candAcc[c * PQ_LAB + (unsigned)l], weight_fx(val[l]));
                } else {
                  credit_wave_sum(fluxAcc + (size_t)l * p.planeStride, q, sel ? weight_fx(val[l]) : 0ull);
                }
              }
            }
          } else if (ABSORB) {
            const unsigned long long m = ballot64(sel);
            if (m && lane == (unsigned)(__ffsll((long long)m) - 1))
              atomicAdd(&fluxAcc[q], (u64)__popcll(m) * 1099511627776ull); // unit weights: count x 2^40
          } else {
            if (sel)
              atomicAdd(&candAcc[c], creditW);
          }
        }
        if (PQ_SUMS) {
          __builtin_amdgcn_wave_barrier();
          if (lane < cands.count) {
            const unsigned q = cands.rec[lane].x;
#pragma unroll
            for (unsigned l = 0; l < PQ_LAB; ++l) {
              const unsigned long long v = *(volatile VR_LDS unsigned long long *)&candAcc[lane * PQ_LAB + l];
              if (v && l < p.numData)
                atomicAdd(&fluxAcc[(size_t)l * p.planeStride + q], v);
            }
          }
        }
      }
    }
    // ---- end of crediting: what is left of the round finishes segments early ----
    if constexpr (FOLLOW) {
      // ---- follow-up segments.  A ray that goes on after this round's event (reflected off the surface, let through
      // a back face, turned round by a side wall) would search the geometry again in the next round — on a flat scene
      // only to leave it at once, and the wave would pay a second packet query for it.  Where the new segment's stretch
      // inside the scene box lies within the box Q of this round's query, the query's candidates are every primitive it
      // can meet (a disk it hits holds a point of that stretch, hence meets Q): they are tested here, and a segment that
      // meets none of them is finished in this round — its wall test and the miss / boundary branches of the state
      // machine (rayTraceKernel.hpp:169-214).  A segment that does meet one is left to the next round as before.
      // Same arithmetic, same closest-hit rule: nothing changes in the results (the parity tests run both ways,
      // VR_DEBUG_FLAGS=256 switches this off).
      if (pqCredit && cands.box && !(p.debugFlags & 256u)) {
        const bool again = fin && active;
        bool inside = false, reaches = false;
        if (again) {
          const U4 ql = cands.rec[VR_PQ_BOX], qh = cands.rec[VR_PQ_BOX + 1];
          const V3 inv = safe_inverse(dir);
          const float tx0 = (p.sceneLo[0] - org.x) * inv.x, tx1 = (p.sceneHi[0] - org.x) * inv.x;
          const float ty0 = (p.sceneLo[1] - org.y) * inv.y, ty1 = (p.sceneHi[1] - org.y) * inv.y;
          const float tz0 = (p.sceneLo[2] - org.z) * inv.z, tz1 = (p.sceneHi[2] - org.z) * inv.z;
          const float tEnter = fmaxf(fminf(tx0, tx1), fminf(ty0, ty1));
          const float tIn = fmaxf(tEnter, fmaxf(fminf(tz0, tz1), tnear));
          const float tQ = fmaxf(tEnter, fmaxf(fminf(tz0, tz1), 0.f));
          const float tOut = fminf(fminf(fmaxf(tx0, tx1), fmaxf(ty0, ty1)), fmaxf(tz0, tz1));
          reaches = tIn <= tOut; // (as pq_hit_packet's `valid`: otherwise no part of the segment is inside the scene box)
          float tBeg = tQ, tEnd = tOut;
          bool capped = false;
          if (RELIEF && !(p.debugFlags & 512u)) {
            // (a reflected ray mostly rises clear of everything near by: the height field's one look-up says so without a
            //  walk.  Otherwise, as the query's own rays: the stretch through the local relief — none: the ray cannot meet
            //  the geometry — by a SHORT walk: a grazing ray that is not through after six tiles is left to the next round,
            //  i.e. to the spill queue; the lanes of a wave walk together, and one such ray kept all of them waiting)
            if (reaches && rises_clear<D>(wallS, org, dir, tnear)) {
              reaches = false;
            } else {
              float tA, tB;
              capped = relief_clip<6>(wallS, reaches, org, dir, tQ, tOut, tA, tB);
              reaches = reaches && tA <= tB;
              tBeg = tA;
              tEnd = tB;
            }
          }
          const float ax = org.x + dir.x * tBeg, ay = org.y + dir.y * tBeg, az = org.z + dir.z * tBeg;
          const float bx = org.x + dir.x * tEnd, by = org.y + dir.y * tEnd, bz = org.z + dir.z * tEnd;
          // (inside Q proper: the padding absorbs the rounding of the clip, as it does for the query's own rays)
          const float pad = p.pqPad;
          const float lx = __uint_as_float(ql.x) + pad, ly = __uint_as_float(ql.y) + pad, lz = __uint_as_float(ql.z) + pad;
          const float hx = __uint_as_float(qh.x) - pad, hy = __uint_as_float(qh.y) - pad, hz = __uint_as_float(qh.z) - pad;
          inside = !capped && (!reaches || (fminf(ax, bx) >= lx && fmaxf(ax, bx) <= hx && fminf(ay, by) >= ly && fmaxf(ay, by) <= hy &&
                                            fminf(az, bz) >= lz && fmaxf(az, bz) <= hz));
          if (RELIEF && (p.debugFlags & 2048u) && !inside) { // EXPERIMENT (wrong results): long continuing rays vanish
            const float ex = bx - ax, ey = by - ay, ez = bz - az;
            if ((ex * ex + ey * ey) + ez * ez > p.reliefTravel * p.reliefTravel)
              active = false;
          }
          if (RELIEF && (p.debugFlags & 4096u) && !inside) // EXPERIMENT (wrong results): every continuing ray not finished here vanishes
            active = false;
        }
        if (ballot64(inside)) {
          bool meets = false;
          if (ballot64(inside && reaches)) {
            for (unsigned c = 0; c < cands.count; ++c) {
              const U4 cr = cands.rec[c], nr = cands.rec[VR_PQ_NRM + c]; // (LDS broadcasts)
              const float4 c4 = make_float4(__uint_as_float(cr.y), __uint_as_float(cr.z), __uint_as_float(cr.w), __uint_as_float(nr.w));
              float t;
              meets = meets || hit_disc(org, dir, tnear, c4, mk(__uint_as_float(nr.x), __uint_as_float(nr.y), __uint_as_float(nr.z)), t);
            }
          }
          if (inside && !(reaches && meets)) {
            HitRec h2;
            hit_clear(h2);
            hit_walls(p, wallS, org, dir, tnear, h2);
            VR_COUNT(K_TRACES, 1);
            if (h2.geom < 0) { // miss, :172-176
              VR_COUNT(K_NONGEO, 1);
              active = false;
            } else { // boundary, :206-214
              const V3 hitPoint = mk(org.x + dir.x * h2.t, org.y + dir.y * h2.t, org.z + dir.z * h2.t);
              if (++boundaryHits > p.maxBoundaryHits) {
                VR_COUNT(K_TERM, 1);
                active = false;
              } else {
                process_boundary_hit<D>(p, wallS, h2.prim, hitPoint, org, rayDirection, dir, active);
              }
            }
            if (!active) {
              VR_COUNT(K_BOUNDARY, boundaryHits);
              VR_COUNT(K_REFL, numReflections);
            }
            start = active;
          }
        }
      }
    }
    if constexpr (FOLLOW && RELIEF) {
      // ---- spill: a ray that would go on into the next round leaves as a full-state record (TraceParams::spillRec);
      // the launch over the loose bins resumes it.  This kernel's waves then hold fresh, sorted rays only.
      if (p.spillRec && !(p.debugFlags & 8192u)) { // (flag 8192: no spilling, for comparison)
        const bool sp = active && start;
        const unsigned long long sm = ballot64(sp);
        if (sm) {
          // (the queue in BLOCKS of 64 records, each filled by one wave: the records of a block are rays of one
          //  neighbourhood — this wave's consecutive rounds — and the resuming kernel takes a block per round; filed in
          //  order of arrival, 8 rays of a round side by side, its waves held rays of eight places.  Only a wave's last
          //  block has unused records: spill_pad at the end of the kernel)
          const unsigned n = (unsigned)__popcll(sm), room = VR_SPILL_BLOCK - spillUsed;
          unsigned nextBase = 0u;
          if (n > room) { // (the block is filled up, the rest of the round's rays open the next one)
            if (lane == 0u)
              nextBase = atomicAdd(p.spillCount, VR_SPILL_BLOCK);
            nextBase = (unsigned)__builtin_amdgcn_readfirstlane((int)nextBase);
          }
          if (sp) {
            const unsigned rank = (unsigned)__popcll(sm & ((1ull << lane) - 1ull));
            float4 *sr = reinterpret_cast<float4 *>(p.spillRec) + 4 * (size_t)(rank < room ? spillBase + spillUsed + rank : nextBase + (rank - room));
            sr[0] = make_float4(org.x, org.y, org.z, rayWeight);
            sr[1] = make_float4(rayDirection.x, rayDirection.y, rayDirection.z, __uint_as_float(rng.seed)); // (the engine's seed: tea3(idx, seed))
            sr[2] = make_float4(__uint_as_float(rng.k), __uint_as_float(numReflections),
                                __uint_as_float(boundaryHits | (hitFromBack ? 0x80000000u : 0u)), 0.f);
            sr[3] = make_float4(__uint_as_float((unsigned)(rng.lo & 0xFFFFFFFFull)), __uint_as_float((unsigned)(rng.lo >> 32)),
                                __uint_as_float((unsigned)(rng.hi & 0xFFFFFFFFull)), __uint_as_float((unsigned)(rng.hi >> 32)));
            active = false;
            start = false;
          }
          spillBase = n > room ? nextBase : spillBase;
          spillUsed = n > room ? n - room : spillUsed + n;
        }
      }
    }
    if constexpr (!ABSORB && !FOLLOW) {
      // ---- segments that rise clear (the general kernels without the packet query's candidate list).  A ray that goes
      // on after this round's event — reflected off the TOP surface of a structure: a fifth of all segments of a trench
      // — used to keep its lane for one more round: a walk of two or three steps while the other lanes walk thirty.
      // The height field over the source plane (HeightFieldParams: per tile the highest point of anything in the tile
      // or its eight neighbours, plus a rounding margin) decides it here: a ray that is above its tile's height from
      // tnear on, and rises above the whole scene before it has travelled a tile sideways, cannot meet the geometry —
      // a primitive it met would hold a point of the ray, hence reach up to the ray's height within those nine tiles.
      // Such a segment is finished in this round: wall test, then the miss / boundary branches of the state machine
      // (rayTraceKernel.hpp:169-214), and its lane pulls a new ray in the next round.  (Not with a mean free path: that
      // scatter is drawn before the boundary branch.  VR_DEBUG_FLAGS=256 switches this off; the tests run both ways.)
      if (!(p.debugFlags & 256u) && !(EXT && EXT_FULL && p.meanFreePath > 0.f)) {
        const bool clear = fin && active && rises_clear<D>(wallS, org, dir, tnear);
        if (clear) {
          HitRec h2;
          hit_clear(h2);
          hit_walls(p, wallS, org, dir, tnear, h2);
          VR_COUNT(K_TRACES, 1);
          if (h2.geom < 0) { // miss, :172-176
            VR_COUNT(K_NONGEO, 1);
            active = false;
          } else { // boundary, :206-214
            const V3 hitPoint = mk(org.x + dir.x * h2.t, org.y + dir.y * h2.t, org.z + dir.z * h2.t);
            if (++boundaryHits > p.maxBoundaryHits) {
              VR_COUNT(K_TERM, 1);
              active = false;
            } else {
              process_boundary_hit<D>(p, wallS, h2.prim, hitPoint, org, rayDirection, dir, active);
            }
          }
          if (!active) {
            VR_COUNT(K_BOUNDARY, boundaryHits);
            VR_COUNT(K_REFL, numReflections);
          }
          start = active;
        }
      }
    }
    TICK(6);
  }
  if constexpr (FOLLOW && RELIEF) {
    if (p.spillRec)
      spill_pad(p, spillBase, spillUsed, lane); // (the unused end of this wave's last block: no rays)
  }

  if (SMALL) {
    // every wave of the block has left the loop: the block's LDS accumulators go to its replica in HBM
    __syncthreads();
    for (unsigned l = 0; l < p.numData + (STATS ? (unsigned)VR_STAT_PLANES : 0u); ++l)
      for (unsigned k = tid; k < p.numPrims; k += VR_BLOCK)
        if (fluxAcc[(size_t)l * p.numPrims + k])
          atomicAdd(&fluxGlobal[(size_t)l * p.planeStride + k], fluxAcc[(size_t)l * p.numPrims + k]);
  }
#ifdef VR_DIAG
  TICK(7);
  if (lane < 16 && phaseT[lane])
    atomicAdd(&p.counters[C_PHASE + lane], phaseT[lane]);
  for (int k = 0; k < 16; ++k) {
    const unsigned long long sw = wave_sum(diagW[k]), sl = wave_sum(diagL[k]);
    if (lane == 0 && sl) {
      atomicAdd(&p.counters[C_DIAG + 2 * k], sw);
      atomicAdd(&p.counters[C_DIAG + 2 * k + 1], sl);
    }
  }
#endif
  // (slot order of vr_types.hpp: traces, nongeo, geo, particle, boundary, reflections, terminated, tier2)
  auto total = [&](int k) -> unsigned { return cnt[k * VR_BLOCK]; }; // this lane's share of counter k
  const unsigned vals[8] = {total(K_TRACES), total(K_NONGEO), total(K_GEO),  total(K_PARTICLE),
                            total(K_BOUNDARY), total(K_REFL), total(K_TERM), total(K_TIER2)};
#undef VR_COUNT
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const unsigned long long s = wave_sum(vals[i]);
    if (lane == 0 && s)
      atomicAdd(&p.counters[i], s);
  }
}

} // namespace vr
