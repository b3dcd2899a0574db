// vr_gather_species.hip — up to four species weighed along ONE set of traced paths (vr_gather_species*; include/
// viennaray_amd.h has the definition, vr_gather.hpp the per-species step and the weight rule, vr_gather_species.cpp the
// host side).  A translation unit of its own beside vr_gather.hip: gather_samples_kernel and its instantiations keep their
// text and their registers; nothing an apply() runs is in here.
//
//   gather_species_kernel<GEO, D, NS, STAT>  the path walk of gather_samples_kernel<GEO, D, false, 3, STAT> — the same
//                                  persistent grid, work items (64 primitives x one chunk or run; lane = primitive),
//                                  chunk engines, samples, segments, wall budget and ends — with NS throughputs per path
//                                  in place of one.  A path's geometry does not depend on the species: the mirror
//                                  direction follows from the normal, the DIFFUSE draw from (seed, primitive, sample,
//                                  bounce).  At a front-side hit every living species takes its own multiplies
//                                  (gather_species_absorb, gather_species_reflect); the path goes on while one is alive.
//                                  At the tail every living species is weighed by its own laws (gather_path_weight_laws)
//                                  and summed into its own exact int64 sum: row s has the bits of the single-species call.
//                                  With STAT and a list (a later round of vr_gather_species_adaptive_device) the lane's
//                                  primitive is a list entry and its paths start with the species of the entry's mask
//                                  alive: one that has met its target is dead from the start — it adds nothing to its
//                                  sums and does not keep the shared path going.
//   gather_species_decide_kernel   one round's verdict of that call: per entry the species of its mask tested each under
//                                  its own targets (vr_gather.hpp: gather_species_decide), the outputs of those that
//                                  leave, the entries with a species left compacted in order with their new masks.
//
// Registers.  The triangle instantiations of the parent sit at 255 VGPRs, the 2-D disks at 166 of 168: NS throughputs and
// NS (2 NS with STAT) int64 sums per lane do not fit beside the walk.  They live in lane-private LDS slots instead —
// [slot][thread of the block], as the walk's stack does: no atomic, no barrier, a bank per lane — and are touched at a
// bounce and at a path's tail only, never inside the walk.  The one thing a lane carries in a register is the mask of
// its living species.  The disk kernels keep the species' scalars in LDS as well (parS, below).  NS is a template parameter and every loop over the species is unrolled: T[] and the look-ups
// index with constants.  NS is 2 or 4; three species run the four-wide kernel with a fourth that is never alive.
#include <hip/hip_runtime.h>

#include "vr_cast.hpp"
#include "vr_gather.hpp"
#include "vr_gather_device.hpp"
#include "vr_kernels.hpp"
#include "vr_trace_kernel.hpp"

namespace vr {

static_assert(GATHER_SPECIES_MAX == GATHER_MAX_SPECIES, "vr_kernels.hpp's bound is vr_gather.hpp's");

// a species' scalars where the block stages them in LDS (parS): rho, g, cosinePower, g_L and the three counts (as bits)
constexpr int PAR_RHO = 0, PAR_G = 1, PAR_N = 2, PAR_GL = 3, PAR_COUNT = 4, SPECIES_PAR = 8;

template <int GEO, int D, int NS, int STAT>
__global__ __launch_bounds__(VR_BLOCK) void gather_species_kernel(const TraceParams p, const GatherSpeciesArgs sa) {
  static_assert(NS == 2 || NS == 4, "two instantiations per (GEO, D, STAT)");
  __shared__ float wallS[VR_WALL_TABLE];
  __shared__ unsigned stackS[VR_STACK_LDS * VR_BLOCK]; // [entry][thread of the block]
  __shared__ float lawBuf[NS * 3 * GATHER_LAW_MAX];    // species s, law w at (3 s + w) x GATHER_LAW_MAX
  __shared__ float tS[NS * VR_BLOCK];                  // [species][thread]: the lane's throughputs
  __shared__ long long sumS[NS * (1 + STAT) * VR_BLOCK]; // [species][thread]: the lane's sums; with STAT the squares behind them
  // The species' scalars are read at a bounce and at a tail only.  From the launch arguments they hold scalar registers
  // for the whole walk; the disk kernels then spill some 60 to 130 of them and end above the parent's VGPR edge, so there
  // the block stages them in LDS and reads them back where they are used.  The triangle kernels are at the VGPR edge
  // either way and lose a wave per SIMD to the extra vector temporaries: they keep the arguments (DESIGN 8w has the table)
  constexpr bool PAR_LDS = GEO == 0;
  __shared__ float parS[PAR_LDS ? NS * SPECIES_PAR : 1];
  const GatherArgs &a = sa.a;
  if constexpr (PAR_LDS) {
    if (threadIdx.x == 0u) {
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        float *par = parS + s * SPECIES_PAR;
        par[PAR_RHO] = sa.rho[s], par[PAR_G] = sa.g[s], par[PAR_N] = sa.cosinePower[s], par[PAR_GL] = sa.gL[s];
#pragma unroll
        for (int w = 0; w < 3; ++w)
          par[PAR_COUNT + w] = __uint_as_float(sa.lawCount[s][w]);
      }
    }
  }
  // (s and the field are constants wherever these are called: the loops over the species are unrolled)
  auto parF = [&](int s, int field) -> float {
    if constexpr (PAR_LDS)
      return parS[s * SPECIES_PAR + field];
    else
      return field == PAR_RHO ? sa.rho[s] : field == PAR_G ? sa.g[s] : field == PAR_N ? sa.cosinePower[s] : sa.gL[s];
  };
  auto parCount = [&](int s, int law) -> uint32_t {
    if constexpr (PAR_LDS)
      return __float_as_uint(parS[s * SPECIES_PAR + PAR_COUNT + law]);
    else
      return sa.lawCount[s][law];
  };
  for (unsigned k = threadIdx.x; k < VR_WALL_TABLE; k += blockDim.x)
    wallS[k] = p.wallTable[k];
  if (sa.laws) { // (block-uniform; absent laws are never read: sa.lawCount says which are there.  sa.num <= NS)
    const unsigned words = min(sa.num, (unsigned)NS) * 3u * GATHER_LAW_MAX;
    for (unsigned k = threadIdx.x; k < words; k += blockDim.x)
      lawBuf[k] = sa.laws[k];
  }
  __syncthreads(); // (the only block-wide point: from here on the waves run on their own)
  const unsigned lane = threadIdx.x & 63u;
  const unsigned wavesPerBlock = blockDim.x >> 6;
  const unsigned wave = blockIdx.x * wavesPerBlock + (threadIdx.x >> 6); // < waves <= the slabs of p.walkStack (launch_gather_species)
  const unsigned waves = gridDim.x * wavesPerBlock;
  unsigned *const stackL = stackS + threadIdx.x;
  unsigned *const stackG = p.walkStack + (size_t)wave * (VR_STACK_GLOBAL * 64u) + lane;
  float *const tL = tS + threadIdx.x;         // species s at tL[s * VR_BLOCK]   (threadIdx.x < blockDim.x <= VR_BLOCK)
  long long *const sumL = sumS + threadIdx.x; // species s at sumL[s * VR_BLOCK], its squares at sumL[(NS + s) * VR_BLOCK]
  const uint4 *__restrict__ pnodes = reinterpret_cast<const uint4 *>(p.pnodes);
  const float4 *__restrict__ prims = reinterpret_cast<const float4 *>(p.prims);
  const GatherFrame frame{p.rayDir, p.firstDir, p.secondDir, -p.posNeg};
  const unsigned allAlive = (1u << min(sa.num, (unsigned)NS)) - 1u; // (a species beyond sa.num is never alive and writes nothing)
#ifdef VR_DIAG
  unsigned long long phaseDummy[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tLast = 0ull;
  unsigned long long *const phaseT = phaseDummy;
#endif
  VR_DIAG_DECL
  const unsigned run = GATHER_CHUNK / a.subs; // samples of a work item: a.subs runs per chunk
  const u64 perGroup = (u64)a.chunks * a.subs, items = (u64)a.groups * perGroup;
  for (u64 it = wave; it < items; it += waves) {
    const unsigned sub = (unsigned)(it % a.subs), chunk = (STAT ? a.chunkFirst : 0u) + (unsigned)((it / a.subs) % a.chunks);
    u64 t = (it / perGroup) * 64u + lane; // index into the range, or (whole scene) the leaf position
    bool valid = t < (u64)a.primCount;
    unsigned startAlive = allAlive; // the species the lane's paths start with
    if constexpr (STAT) {
      if (a.list) { // (wave-uniform; a later round of the adaptive call) the lane's primitive is the list's — entries <
                    // a.primCount — and its paths start with the species still sampling there (gather_species_decide_kernel)
        valid = t < (u64)a.listCount;
        startAlive = valid ? sa.listMask[t] & allAlive : 0u;
        t = valid ? a.list[t] : 0u;
      }
    }
    // ---- the lane's primitive ----
    GVec o = GVec{0.f, 0.f, 0.f}, m = GVec{0.f, 0.f, 1.f};
    unsigned orig = 0u;
    if (valid) {
      const unsigned q = a.leafOfOrig ? a.leafOfOrig[a.primFirst + (unsigned)t] : (unsigned)t;
      gather_primitive<GEO>(prims, q, o, m, orig);
      if (a.leafOfOrig)
        orig = a.primFirst + (unsigned)t; // (what the record says; taken from the range so that the accumulator's index is in it)
    }
    const unsigned count = min(GATHER_CHUNK, a.samples - chunk * GATHER_CHUNK); // samples of this chunk: wave-uniform
    // ---- the chunk's engine: outputs 0 and 1, then the streaming cursors ----
    u64 out[2], lo, hi;
    mt_first_outputs<2>(gather_chunk_seed(orig, a.seed, chunk), out, lo, hi);
    unsigned k = 2u;
    float r1 = gather_canon(out[0]), r2 = gather_canon(out[1]);
    // ---- this item's run of the chunk: samples jFirst .. jEnd - 1 (the draws of those before it are stepped over) ----
    const unsigned jFirst = sub * run, jEnd = min(count, jFirst + run);
    for (unsigned j = 0; j < jFirst; ++j) {
      r1 = gather_canon(gather_draw(k, lo, hi));
      r2 = gather_canon(gather_draw(k, lo, hi));
    }
#pragma unroll
    for (int s = 0; s < NS * (1 + STAT); ++s)
      sumL[s * VR_BLOCK] = 0;
    for (unsigned j = jFirst; j < jEnd; ++j) {
      const GVec w0 = gather_direction(GATHER_NORMAL, D, r1, r2, m, 1.f, frame);
      const float c = gather_c(w0, frame), mDotW = gather_dot(m, w0);
      V3 org = v3(o), rayDirection = v3(w0), dir = project_dir<D>(rayDirection);
      bool active = valid;
      const bool walked = active;
      CastState cs;
      cast_begin(cs);
      bool ignored = false;
      unsigned hitPos = 0u;
      float cEnd = c;           // u . omega of the direction the path goes along
      unsigned bounces = 0u;
      unsigned alive = startAlive; // the species that still follow the path
#pragma unroll
      for (int s = 0; s < NS; ++s)
        tL[s * VR_BLOCK] = 1.f;
      // ---- segments, until every sample of the wave has ended ----
      while (ballot64(active)) {
        HitRec h;
        hit_clear(h);
        unsigned node = 0u, sp = 0u;
        pair_walk_lanes<GEO, VR_STACK_LDS>(p, pnodes, prims, stackL, stackG, active, org, dir, VR_GATHER_TNEAR, h, node, sp, 1u VR_DIAG_PASS);
        if (active) {
          hit_walls(p, wallS, org, dir, VR_GATHER_TNEAR, h);
          const V3 hitPoint = mk(org.x + dir.x * h.t, org.y + dir.y * h.t, org.z + dir.z * h.t);
          hitPos = h.pos;
          if (cast_segment(cs, h.geom, h.prim, h.t, true, a.maxBoundaryHits, __builtin_huge_valf()) == CAST_AT_WALL) {
            process_boundary_hit<D>(p, wallS, h.prim, hitPoint, org, rayDirection, dir, active);
            if (!active) {
              cast_ignored(cs);
              ignored = true;
            }
          } else {
            active = false;
            // the step of a path at a geometry hit, in gather_bounce's order: a back side and the bounce budget end the path
            // for every species; then every living species takes its rho; the leaving direction is formed once if one is
            // left; then the reflectivity laws at mu = n_j . leaving
            if (cs.prim >= 0) {
              const V3 nj = gather_hit_normal<GEO>(prims, hitPos);
              if (vdot(dir, nj) < 0.f && bounces < a.maxBounces) {
                float T[NS], rho[NS];
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                  T[s] = tL[s * VR_BLOCK];
                  rho[s] = parF(s, PAR_RHO);
                  if (sa.rhoLeaf[s]) // (wave-uniform; hitPos < numPrims: a leaf position the walk returned)
                    rho[s] = sa.rhoLeaf[s][hitPos];
                }
                alive = gather_species_absorb<NS>(T, alive, rho);
                if (alive) {
                  V3 leaving;
                  if (a.reflection == GATHER_REFLECT_SPECULAR) // (wave-uniform)
                    leaving = reflect_specular(rayDirection, nj);
                  else
                    leaving = v3(gather_path_diffuse(D, a.seed, orig, chunk * GATHER_CHUNK + j, bounces, GVec{nj.x, nj.y, nj.z}));
                  if (sa.laws) { // (wave-uniform)
                    const float *R[NS];
                    uint32_t MR[NS];
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                      R[s] = lawBuf + (3 * s + GATHER_LAW_REFLECTIVITY) * GATHER_LAW_MAX;
                      MR[s] = parCount(s, GATHER_LAW_REFLECTIVITY);
                    }
                    alive = gather_species_reflect<NS>(T, alive, R, MR, vdot(nj, leaving));
                  }
                  if (alive) {
                    rayDirection = leaving;
                    dir = project_dir<D>(rayDirection);
                    org = hitPoint; // (org + dir * t: the tracer's restart)
                    cEnd = gather_c(GVec{rayDirection.x, rayDirection.y, rayDirection.z}, frame);
                    ++bounces;
                    active = true;
                  }
                }
#pragma unroll
                for (int s = 0; s < NS; ++s)
                  tL[s * VR_BLOCK] = T[s];
              }
            }
          }
        }
      }
      // ---- the tail: a path that ended on a primitive weighs 0 for every species, like one stopped on a wall ----
      if (walked) {
        const int tailEnd = cs.prim == CAST_MISS ? (ignored ? GATHER_END_IGNORED : GATHER_END_MISS) : GATHER_END_WALL;
        if (tailEnd == GATHER_END_MISS) { // (every other end weighs 0 whatever the species: nothing to add)
#pragma unroll
          for (int s = 0; s < NS; ++s) {
            if (!((alive >> s) & 1u)) // (a dead species weighs 0: it is not weighed from a T of 0)
              continue;
            const uint32_t nL = parCount(s, GATHER_LAW_SOURCE), nY = parCount(s, GATHER_LAW_YIELD);
            const float *L = lawBuf + (3 * s) * GATHER_LAW_MAX;
            const float w = gather_path_weight_laws(
                tailEnd, parF(s, PAR_G), parF(s, PAR_N), cEnd, tL[s * VR_BLOCK], nL ? L + GATHER_LAW_SOURCE * GATHER_LAW_MAX : nullptr, nL,
                parF(s, PAR_GL), nY ? L + GATHER_LAW_YIELD * GATHER_LAW_MAX : nullptr, nY, mDotW);
            sumL[s * VR_BLOCK] += gather_q(w, a.wmax);
            if constexpr (STAT)
              sumL[(NS + s) * VR_BLOCK] += gather_q2(w, a.wmax);
          }
        }
      }
      if (j + 1u < jEnd) { // outputs 2 (j + 1) and 2 (j + 1) + 1
        r1 = gather_canon(gather_draw(k, lo, hi));
        r2 = gather_canon(gather_draw(k, lo, hi));
      }
    }
    // (orig - primFirst < primCount: valid; s < sa.num: inside the num x primCount sums)
    if (valid) {
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        if ((unsigned)s >= sa.num)
          continue;
        const size_t idx = (size_t)s * a.primCount + (orig - a.primFirst);
        const long long sum = sumL[s * VR_BLOCK];
        if (sum != 0)
          atomicAdd(a.acc + idx, (unsigned long long)sum);
        if constexpr (STAT) {
          const long long sumSq = sumL[(NS + s) * VR_BLOCK];
          if (sumSq != 0)
            atomicAdd(a.accSq + idx, (unsigned long long)sumSq);
        }
      }
    }
  }
}

// One round's verdict of vr_gather_species_adaptive_device: gather_decide_kernel's shape — one thread per entry of the
// current list, a block per GATHER_DECIDE_BLOCK entries, the next list in the order of the current one by wave ballots and
// a block prefix, no atomic append — with a mask of species per entry.  Only the species of the entry's mask are loaded
// and tested: one outside it stopped at an older K.  WRITE false: the block's count alone, for a list of more than one
// block; WRITE true: the outputs, the next list and its masks, the list's length, and per species the entries it is left
// in (one atomic per wave and species: a count, not a place)
template <bool WRITE> __global__ __launch_bounds__(GATHER_DECIDE_BLOCK) void gather_species_decide_kernel(const GatherSpeciesDecideArgs d) {
  __shared__ unsigned waveCount[GATHER_DECIDE_BLOCK / 64];
  __shared__ unsigned red[GATHER_DECIDE_BLOCK];
  const unsigned e = blockIdx.x * GATHER_DECIDE_BLOCK + threadIdx.x; // (count <= 2^32 - 1: a primitive range)
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const bool have = e < d.count;
  unsigned entry = 0u, idx = 0u, mask = 0u, failed = 0u, writes = 0u;
  int64_t S1[GATHER_SPECIES_MAX] = {0, 0, 0, 0}, S2[GATHER_SPECIES_MAX] = {0, 0, 0, 0};
  if (have) {
    entry = d.list ? d.list[e] : e;
    idx = d.origWords ? d.origWords[(size_t)entry * d.origStride + d.origOffset] : entry; // < primCount
    mask = (d.masks ? d.masks[e] : ~0u) & ((1u << d.num) - 1u);
#pragma unroll
    for (unsigned s = 0; s < GATHER_SPECIES_MAX; ++s)
      if (s < d.num && ((mask >> s) & 1u)) { // (s < num, idx < primCount: inside the num x primCount sums)
        S1[s] = (int64_t)d.acc[(size_t)s * d.primCount + idx];
        S2[s] = (int64_t)d.accSq[(size_t)s * d.primCount + idx];
      }
    failed = gather_species_decide(S1, S2, d.num, d.samples, d.rel, d.abs, mask, d.last != 0u, writes);
  }
  const bool keep = failed != 0u;
  const unsigned long long kept = ballot64(keep);
  if (lane == 0u)
    waveCount[wave] = (unsigned)__popcll(kept);
  if constexpr (WRITE) { // the kept entries of the blocks before this one
    unsigned part = 0u;
    for (unsigned b = threadIdx.x; b < blockIdx.x; b += GATHER_DECIDE_BLOCK)
      part += d.blockCounts[b];
    red[threadIdx.x] = part;
  }
  __syncthreads();
  unsigned before = 0u, total = 0u;
  for (unsigned w = 0; w < GATHER_DECIDE_BLOCK / 64; ++w) {
    const unsigned n = waveCount[w];
    before += w < wave ? n : 0u;
    total += n;
  }
  if constexpr (!WRITE) {
    if (threadIdx.x == 0u)
      d.blockCounts[blockIdx.x] = total;
  } else {
    for (unsigned s = GATHER_DECIDE_BLOCK / 2; s > 0u; s >>= 1) {
      if (threadIdx.x < s)
        red[threadIdx.x] += red[threadIdx.x + s];
      __syncthreads();
    }
    const unsigned base = red[0];
#pragma unroll
    for (unsigned s = 0; s < GATHER_SPECIES_MAX; ++s) {
      const unsigned long long left = ballot64(((failed >> s) & 1u) != 0u); // (every lane of the wave is here)
      if (lane == 0u && left)
        atomicAdd(d.words + 1u + s, (unsigned)__popcll(left));
    }
    if (have) {
#pragma unroll
      for (unsigned s = 0; s < GATHER_SPECIES_MAX; ++s)
        if ((writes >> s) & 1u) { // (writes is a subset of the mask: s < num)
          const size_t o = (size_t)s * d.primCount + idx;
          d.flux[o] = gather_result(S1[s], d.samples);
          if (d.stdErr)
            d.stdErr[o] = (float)sqrt(gather_stderr2(S1[s], S2[s], d.samples));
          if (d.samplesUsed)
            d.samplesUsed[o] = d.samples;
        }
      if (keep) { // (base + before + the lanes before < the kept entries of the whole list <= count: inside next / nextMasks)
        const unsigned at = base + before + (unsigned)__popcll(kept & ((1ull << lane) - 1ull));
        d.next[at] = entry;
        d.nextMasks[at] = failed;
      }
    }
    if (blockIdx.x == gridDim.x - 1u && threadIdx.x == 0u)
      d.words[0] = base + total;
  }
}

template <int NS, int STAT>
static void species_launch(int geo, int D, dim3 g, dim3 b, hipStream_t st, const TraceParams &p, const GatherSpeciesArgs &sa) {
  if (geo == 0) {
    if (D == 2)
      hipLaunchKernelGGL((gather_species_kernel<0, 2, NS, STAT>), g, b, 0, st, p, sa);
    else
      hipLaunchKernelGGL((gather_species_kernel<0, 3, NS, STAT>), g, b, 0, st, p, sa);
  } else {
    if (D == 2)
      hipLaunchKernelGGL((gather_species_kernel<1, 2, NS, STAT>), g, b, 0, st, p, sa);
    else
      hipLaunchKernelGGL((gather_species_kernel<1, 3, NS, STAT>), g, b, 0, st, p, sa);
  }
}

hipError_t launch_gather_species(const TraceParams &p, int geo, int D, const GatherSpeciesArgs &sa, unsigned slabs, hipStream_t st) {
  const GatherArgs &a = sa.a;
  // what the kernel relies on: the launch shape of launch_gather_samples, a path gather's arguments, 2 .. 4 species with
  // reflectivities, counts and tables the look-ups may index
  if (a.subs == 0 || a.subs > GATHER_MAX_SUBS || (a.subs & (a.subs - 1u)))
    return hipErrorInvalidValue;
  if (sa.num < 2u || sa.num > GATHER_SPECIES_MAX || !a.acc || a.paths != 1u || a.links || a.emission || a.laws ||
      a.mode != GATHER_NORMAL || a.reflection > GATHER_REFLECT_DIFFUSE || a.maxBounces > GATHER_MAX_BOUNCES)
    return hipErrorInvalidValue;
  // a list goes with the sums alone, has its masks beside it and is no longer than the range (its entries index the range)
  if (a.list ? !a.stat || !sa.listMask || a.listCount > a.primCount || a.groups != (uint32_t)(((unsigned long long)a.listCount + 63u) / 64u)
             : sa.listMask != nullptr)
    return hipErrorInvalidValue;
  if (a.stat && (!a.accSq || (unsigned long long)(a.chunkFirst + (unsigned long long)a.chunks) * GATHER_CHUNK > a.samples))
    return hipErrorInvalidValue;
  for (unsigned s = 0; s < sa.num; ++s)
    for (int w = 0; w < 3; ++w)
      if (sa.lawCount[s][w] && (!sa.laws || !gather_law_count_ok(sa.lawCount[s][w])))
        return hipErrorInvalidValue;
  const unsigned long long items = (unsigned long long)a.groups * a.chunks * a.subs;
  const unsigned perBlock = VR_BLOCK / 64;
  unsigned waves = items < slabs ? (unsigned)items : slabs;
  if (waves > perBlock)
    waves -= waves % perBlock;
  if (waves == 0)
    return hipSuccess;
  const dim3 g(waves > perBlock ? waves / perBlock : 1u), b(waves > perBlock ? (unsigned)VR_BLOCK : waves * 64u);
  if (sa.num <= 2u) {
    if (a.stat)
      species_launch<2, 1>(geo, D, g, b, st, p, sa);
    else
      species_launch<2, 0>(geo, D, g, b, st, p, sa);
  } else {
    if (a.stat)
      species_launch<4, 1>(geo, D, g, b, st, p, sa);
    else
      species_launch<4, 0>(geo, D, g, b, st, p, sa);
  }
  return hipGetLastError();
}

hipError_t launch_gather_species_decide(const GatherSpeciesDecideArgs &d, hipStream_t st) {
  if (d.count == 0 || d.count > d.primCount || d.num < 2u || d.num > GATHER_SPECIES_MAX || !d.acc || !d.accSq || !d.next ||
      !d.nextMasks || !d.blockCounts || !d.words || !d.flux || d.samples < 2u || (d.masks && !d.list))
    return hipErrorInvalidValue;
  // one launch where the list fits a block, otherwise the blocks' counts first
  const unsigned blocks = (unsigned)(((unsigned long long)d.count + GATHER_DECIDE_BLOCK - 1u) / GATHER_DECIDE_BLOCK);
  if (blocks > 1u)
    hipLaunchKernelGGL((gather_species_decide_kernel<false>), dim3(blocks), dim3(GATHER_DECIDE_BLOCK), 0, st, d);
  hipLaunchKernelGGL((gather_species_decide_kernel<true>), dim3(blocks), dim3(GATHER_DECIDE_BLOCK), 0, st, d);
  return hipGetLastError();
}

} // namespace vr
