// vr_gather_energy.hip — an ion's energy carried along the paths of an angular gather (vr_gather_energy*; include/
// viennaray_amd.h has the definition, vr_gather.hpp the arithmetic — gather_energy_* — vr_gather_energy.cpp the host
// side).  A translation unit of its own beside vr_gather.hip and vr_gather_species.hip: gather_samples_kernel and its
// instantiations keep their text and their registers; nothing an apply() runs is in here.
//
//   gather_energy_kernel<GEO, D, STAT, ONE>  the path walk of gather_samples_kernel<GEO, D, false, 3, STAT> — the same
//                                  persistent grid, work items (64 primitives x one chunk or run; lane = primitive),
//                                  chunk engines, samples, segments, wall budget, ends, throughput and angular weight —
//                                  with two more floats per path: E0, the energy the ion left the source with (a counter
//                                  draw of the path's key read through the source's quantiles), and P, the product of
//                                  the retention law at every vertex the path goes on from.  At the tail the angular
//                                  weight takes one more multiply, by the energy yield at e = (E0 P) / energyMax.
//                                  With the cut (ea.zeros >= 2) a path ends, weighing 0, as soon as e lies where the
//                                  yield reads exactly 0 (gather_energy_cut): before the walk — such a sample is not
//                                  walked at all — and after every update of P.  e never rises, so no bit of any sum
//                                  changes.
//                                  With ONE it writes one path vertex by vertex (vr_debug_gather_energy_path): the same
//                                  loop, of which lane 0 walks ea.a.pathSample alone.
//   gather_energy_put_kernel       the energy tables of a call, from the launch arguments into device memory.
//
// Registers.  The triangle instantiations of the parent sit at 255 VGPRs.  E0 and P live in lane-private LDS slots —
// [slot][thread of the block], as the walk's stack does: no atomic, no barrier, a bank per lane — and are touched at a
// bounce and at a path's tail only, never inside the walk.  The energy tables are staged in LDS beside the angular laws.
#include <hip/hip_runtime.h>

#include "vr_cast.hpp"
#include "vr_gather.hpp"
#include "vr_gather_device.hpp"
#include "vr_kernels.hpp"
#include "vr_trace_kernel.hpp"

namespace vr {

// vertex v of the path vr_debug_gather_energy_path records (vr_gather.hip: gather_path_put has the row)
__device__ __forceinline__ void energy_path_put(const GatherArgs &a, unsigned v, unsigned id, const V3 &pt, const V3 &in, const V3 &n,
                                                const V3 &outDir) {
  if (v >= a.pathMaxVertices)
    return;
  float *row = a.pathVertices + (size_t)v * GATHER_PATH_ROW;
  row[0] = __uint_as_float(id);
  row[1] = pt.x, row[2] = pt.y, row[3] = pt.z;
  row[4] = in.x, row[5] = in.y, row[6] = in.z;
  row[7] = n.x, row[8] = n.y, row[9] = n.z;
  row[10] = outDir.x, row[11] = outDir.y, row[12] = outDir.z;
}

template <int GEO, int D, int STAT, bool ONE = false>
__global__ __launch_bounds__(VR_BLOCK) void gather_energy_kernel(const TraceParams p, const GatherEnergyArgs ea) {
  static_assert(!(STAT && ONE), "the one-path walk sums nothing");
  __shared__ float wallS[VR_WALL_TABLE];
  __shared__ unsigned stackS[VR_STACK_LDS * VR_BLOCK]; // [entry][thread of the block]
  __shared__ float lawBuf[3 * GATHER_LAW_MAX];         // the angular laws, as the parent stages them
  __shared__ float energyBuf[3 * GATHER_LAW_MAX];      // yield, quantiles, retention
  __shared__ float eS[2 * VR_BLOCK];                   // [slot][thread]: the lane's E0 and P
  const GatherArgs &a = ea.a;
  for (unsigned k = threadIdx.x; k < VR_WALL_TABLE; k += blockDim.x)
    wallS[k] = p.wallTable[k];
  if (a.laws) // (block-uniform; absent laws are never read: a.lawCount says which are there)
    for (unsigned k = threadIdx.x; k < 3 * GATHER_LAW_MAX; k += blockDim.x)
      lawBuf[k] = a.laws[k];
  for (unsigned k = threadIdx.x; k < 3 * GATHER_LAW_MAX; k += blockDim.x)
    energyBuf[k] = ea.tables[k];
  __syncthreads(); // (the only block-wide point: from here on the waves run on their own)
  const float *const lawS = lawBuf;
  const float *const yieldS = energyBuf + GATHER_ENERGY_YIELD * GATHER_LAW_MAX;
  const float *const quantS = energyBuf + GATHER_ENERGY_QUANTILES * GATHER_LAW_MAX;
  const float *const retainS = energyBuf + GATHER_ENERGY_RETENTION * GATHER_LAW_MAX;
  const unsigned lane = threadIdx.x & 63u;
  const unsigned wavesPerBlock = blockDim.x >> 6;
  const unsigned wave = blockIdx.x * wavesPerBlock + (threadIdx.x >> 6); // < waves <= the slabs of p.walkStack (launch_gather_energy)
  const unsigned waves = gridDim.x * wavesPerBlock;
  unsigned *const stackL = stackS + threadIdx.x;
  unsigned *const stackG = p.walkStack + (size_t)wave * (VR_STACK_GLOBAL * 64u) + lane;
  float *const e0L = eS + threadIdx.x, *const pL = eS + VR_BLOCK + threadIdx.x; // (threadIdx.x < blockDim.x <= VR_BLOCK)
  const uint4 *__restrict__ pnodes = reinterpret_cast<const uint4 *>(p.pnodes);
  const float4 *__restrict__ prims = reinterpret_cast<const float4 *>(p.prims);
  const GatherFrame frame{p.rayDir, p.firstDir, p.secondDir, -p.posNeg};
  const uint32_t nYE = ea.count[GATHER_ENERGY_YIELD], nQ = ea.count[GATHER_ENERGY_QUANTILES], nEps = ea.count[GATHER_ENERGY_RETENTION];
  const bool cut = ea.zeros >= 2u; // (wave-uniform)
#ifdef VR_DIAG
  unsigned long long phaseDummy[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tLast = 0ull;
  unsigned long long *const phaseT = phaseDummy;
#endif
  VR_DIAG_DECL
  const unsigned run = GATHER_CHUNK / a.subs; // samples of a work item: a.subs runs per chunk
  const u64 perGroup = (u64)a.chunks * a.subs, items = (u64)a.groups * perGroup;
  for (u64 it = wave; it < items; it += waves) {
    const unsigned sub = (unsigned)(it % a.subs), chunk = (STAT ? a.chunkFirst : 0u) + (unsigned)((it / a.subs) % a.chunks);
    if constexpr (ONE) {
      if (chunk != a.pathSample / GATHER_CHUNK) // (wave-uniform) only the chunk that holds the one sample is looked at
        continue;
    }
    u64 t = (it / perGroup) * 64u + lane; // index into the range, or (whole scene) the leaf position
    bool valid = t < (u64)a.primCount;
    if constexpr (STAT) {
      if (a.list) { // (wave-uniform) the lane's primitive is the list's: entries < a.primCount (gather_decide_kernel)
        valid = t < (u64)a.listCount;
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
    long long sum = 0;
    [[maybe_unused]] long long sumSq = 0; // (STAT)
    for (unsigned j = jFirst; j < jEnd; ++j) {
      const GVec w0 = gather_direction(GATHER_NORMAL, D, r1, r2, m, a.cosinePower, frame);
      const float c = gather_c(w0, frame), mDotW = gather_dot(m, w0);
      V3 org = v3(o), rayDirection = v3(w0), dir = project_dir<D>(rayDirection);
      bool starts = valid;
      if constexpr (ONE)
        starts = starts && lane == 0u && chunk * GATHER_CHUNK + j == a.pathSample;
      // ---- the path's energy at the source; the cut's first test, at P = 1: such a sample is not walked at all ----
      bool cutNow = false;
      [[maybe_unused]] float uOne = 0.f; // (ONE) the energy draw
      if (starts) {
        float u = 0.f;
        if (nQ || ONE) // (wave-uniform) a monoenergetic source draws nothing
          u = gather_energy_u(gather_path_key(a.seed, orig, chunk * GATHER_CHUNK + j));
        const float E0 = gather_energy_source(nQ ? quantS : nullptr, nQ, u, ea.sourceEnergy);
        *e0L = E0;
        *pL = 1.f;
        if (cut)
          cutNow = gather_energy_cut(gather_energy_arrival(E0, 1.f, ea.energyMax), nYE, ea.zeros);
        if constexpr (ONE)
          uOne = u;
      }
      bool active = starts && !cutNow;
      CastState s;
      cast_begin(s);
      bool ignored = false;
      unsigned hitPos = 0u;
      float T = 1.f, cEnd = c; // the throughput, and u . omega of the direction the path goes along
      unsigned bounces = 0u;
      [[maybe_unused]] unsigned pathCount = 1u; // (ONE) vertices so far: vertex 0 is the primitive itself
      [[maybe_unused]] int pathEnd = cutNow ? GATHER_END_ENERGY : GATHER_END_MISS;
      if constexpr (ONE) {
        if (starts)
          energy_path_put(a, 0u, orig, org, mk(__int_as_float(0x7FC00000), __int_as_float(0x7FC00000), __int_as_float(0x7FC00000)),
                          v3(m), rayDirection);
      }
      // ---- segments, until every sample of the wave has ended ----
      while (ballot64(active)) {
        HitRec h;
        hit_clear(h);
        unsigned node = 0u, sp = 0u;
        pair_walk_lanes<GEO, VR_STACK_LDS>(p, pnodes, prims, stackL, stackG, active, org, dir, VR_GATHER_TNEAR, h, node, sp, 1u VR_DIAG_PASS);
        if (active) {
#ifdef VR_DIAG
          DIAG(0); // (one wave-iteration per round of segments, one lane-iteration per segment walked in it)
#endif
          hit_walls(p, wallS, org, dir, VR_GATHER_TNEAR, h);
          const V3 hitPoint = mk(org.x + dir.x * h.t, org.y + dir.y * h.t, org.z + dir.z * h.t);
          hitPos = h.pos;
          if (cast_segment(s, h.geom, h.prim, h.t, true, a.maxBoundaryHits, __builtin_huge_valf()) == CAST_AT_WALL) {
            process_boundary_hit<D>(p, wallS, h.prim, hitPoint, org, rayDirection, dir, active);
            if (!active) {
              cast_ignored(s);
              ignored = true;
            }
          } else {
            active = false;
            // the step of a path at a geometry hit, in the order of the parent's (vr_gather.hip: gather_bounce): a back
            // side and the bounce budget end the path; T takes rho; the leaving direction is formed; T takes the
            // reflectivity law at mu = n_j . leaving; then — the path goes on — P takes the retention law at the same mu
            if (s.prim >= 0) {
              int end = GATHER_END_FRONT;
              const V3 nj = gather_hit_normal<GEO>(prims, hitPos);
              [[maybe_unused]] const V3 arriving = rayDirection;
              // (ONE) the direction the retention's mu was read at: recorded where the path goes on and where the cut ends it
              [[maybe_unused]] V3 leftAlong = mk(__int_as_float(0x7FC00000), __int_as_float(0x7FC00000), __int_as_float(0x7FC00000));
              if (!(vdot(dir, nj) < 0.f)) {
                end = GATHER_END_BACK;
              } else if (bounces >= a.maxBounces) {
                end = GATHER_END_BOUNCES;
              } else {
                float rho = a.rho;
                if (a.rhoLeaf)
                  rho = a.rhoLeaf[hitPos]; // (hitPos < numPrims: a leaf position the walk returned)
                T = gather_path_throughput(T, rho);
                if (T == 0.f) {
                  end = GATHER_END_ABSORBED;
                } else {
                  V3 leaving;
                  if (a.reflection == GATHER_REFLECT_SPECULAR) // (wave-uniform)
                    leaving = reflect_specular(rayDirection, nj);
                  else
                    leaving = v3(gather_path_diffuse(D, a.seed, orig, chunk * GATHER_CHUNK + j, bounces, GVec{nj.x, nj.y, nj.z}));
                  const float mu = vdot(nj, leaving);
                  if (a.lawCount[GATHER_LAW_REFLECTIVITY]) // (wave-uniform)
                    T = gather_path_throughput_law(T, lawS + GATHER_LAW_REFLECTIVITY * GATHER_LAW_MAX, a.lawCount[GATHER_LAW_REFLECTIVITY], mu);
                  if (T == 0.f) {
                    end = GATHER_END_ABSORBED;
                  } else {
                    bool goesOn = true;
                    if constexpr (ONE)
                      leftAlong = leaving;
                    if (nEps) { // (wave-uniform)
                      const float P = gather_energy_retain(*pL, retainS, nEps, mu);
                      *pL = P;
                      if (cut && gather_energy_cut(gather_energy_arrival(*e0L, P, ea.energyMax), nYE, ea.zeros)) {
                        end = GATHER_END_ENERGY;
                        goesOn = false;
                      }
                    }
                    if (goesOn) {
                      rayDirection = leaving;
                      dir = project_dir<D>(rayDirection);
                      org = hitPoint; // (org + dir * t: the tracer's restart)
                      cEnd = gather_c(GVec{rayDirection.x, rayDirection.y, rayDirection.z}, frame);
                      ++bounces;
                      active = true;
                    }
                  }
                }
              }
              if constexpr (ONE) {
                energy_path_put(a, pathCount, (unsigned)s.prim, hitPoint, arriving, nj, leftAlong);
                ++pathCount;
                pathEnd = end;
              }
            }
          }
        }
      }
      // ---- the tail: the angular weight, then the last multiply.  A path that ended on a primitive weighs 0 like one
      // stopped on a wall; one the cut ended before its walk weighs 0 as well ----
      if (starts) {
        const int tailEnd = cutNow ? GATHER_END_ENERGY
                                   : (s.prim == CAST_MISS ? (ignored ? GATHER_END_IGNORED : GATHER_END_MISS) : GATHER_END_WALL);
        float w = 0.f;
        [[maybe_unused]] float eOne = 0.f;
        if (tailEnd == GATHER_END_MISS || ONE) { // (every other end weighs 0: 0 times a finite yield)
          const float e = gather_energy_arrival(*e0L, *pL, ea.energyMax);
          w = gather_path_weight_laws(tailEnd, a.g, a.cosinePower, cEnd, T,
                                      a.lawCount[GATHER_LAW_SOURCE] ? lawS + GATHER_LAW_SOURCE * GATHER_LAW_MAX : nullptr,
                                      a.lawCount[GATHER_LAW_SOURCE], a.gL,
                                      a.lawCount[GATHER_LAW_YIELD] ? lawS + GATHER_LAW_YIELD * GATHER_LAW_MAX : nullptr,
                                      a.lawCount[GATHER_LAW_YIELD], mDotW);
          w = gather_energy_weight(w, yieldS, nYE, e);
          if constexpr (ONE)
            eOne = e;
        }
        if constexpr (!ONE) {
          sum += gather_q(w, a.wmax);
          if constexpr (STAT)
            sumSq += gather_q2(w, a.wmax);
        } else { // (lane 0, the one sample)
          const int end = s.prim >= 0 || cutNow ? pathEnd : tailEnd;
          a.pathTail[0] = __uint_as_float(pathCount);
          a.pathTail[1] = __uint_as_float((unsigned)end);
          a.pathTail[2] = rayDirection.x, a.pathTail[3] = rayDirection.y, a.pathTail[4] = rayDirection.z;
          a.pathTail[5] = T;
          a.pathTail[6] = w; // (0 for a path that ended on a primitive: the tail's rule)
          ea.pathEnergy[0] = uOne, ea.pathEnergy[1] = *e0L, ea.pathEnergy[2] = *pL, ea.pathEnergy[3] = eOne;
        }
      }
      if (j + 1u < jEnd) { // outputs 2 (j + 1) and 2 (j + 1) + 1
        r1 = gather_canon(gather_draw(k, lo, hi));
        r2 = gather_canon(gather_draw(k, lo, hi));
      }
    }
    if constexpr (!ONE) {
      if (valid && sum != 0)
        atomicAdd(a.acc + (orig - a.primFirst), (unsigned long long)sum);
      if constexpr (STAT) {
        if (valid && sumSq != 0)
          atomicAdd(a.accSq + (orig - a.primFirst), (unsigned long long)sumSq);
      }
    }
  }
#ifdef VR_DIAG
  { // the rounds of segments and the segments walked in them, as the parent counts them
    const unsigned long long sw = wave_sum(diagW[0]), sl = wave_sum(diagL[0]);
    if (lane == 0u && sl) {
      atomicAdd(&p.counters[C_DIAG], sw);
      atomicAdd(&p.counters[C_DIAG + 1], sl);
    }
  }
#endif
}

// the energy tables of a call from the launch's own arguments (3 KiB of them) into the table the kernel stages: no host
// buffer has to outlive the call, and the write is ordered on the stream like any kernel
struct GatherEnergyTable {
  float v[3 * GATHER_LAW_MAX];
};
__global__ void gather_energy_put_kernel(const GatherEnergyTable t, float *dst) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 3 * GATHER_LAW_MAX)
    dst[i] = t.v[i];
}

// what the kernel relies on: a path gather's arguments, angular laws and energy tables the look-ups may index
static bool gather_energy_ok(const GatherEnergyArgs &ea) {
  const GatherArgs &a = ea.a;
  if (a.subs == 0 || a.subs > GATHER_MAX_SUBS || (a.subs & (a.subs - 1u)))
    return false;
  if (!a.acc || a.paths != 1u || a.links || a.emission || a.mode != GATHER_NORMAL || a.reflection > GATHER_REFLECT_DIFFUSE ||
      a.maxBounces > GATHER_MAX_BOUNCES)
    return false;
  for (int w = 0; w < 3; ++w) {
    if (a.lawCount[w] && (!a.laws || !gather_law_count_ok(a.lawCount[w])))
      return false;
    if (ea.count[w] && !gather_law_count_ok(ea.count[w]))
      return false;
  }
  // the yield is there; the cut's Z0 counts entries of it
  return ea.tables && ea.count[GATHER_ENERGY_YIELD] && ea.zeros <= ea.count[GATHER_ENERGY_YIELD] && ea.energyMax > 0.f;
}

template <int STAT>
static void energy_launch(int geo, int D, dim3 g, dim3 b, hipStream_t st, const TraceParams &p, const GatherEnergyArgs &ea) {
  if (geo == 0) {
    if (D == 2)
      hipLaunchKernelGGL((gather_energy_kernel<0, 2, STAT>), g, b, 0, st, p, ea);
    else
      hipLaunchKernelGGL((gather_energy_kernel<0, 3, STAT>), g, b, 0, st, p, ea);
  } else {
    if (D == 2)
      hipLaunchKernelGGL((gather_energy_kernel<1, 2, STAT>), g, b, 0, st, p, ea);
    else
      hipLaunchKernelGGL((gather_energy_kernel<1, 3, STAT>), g, b, 0, st, p, ea);
  }
}

hipError_t launch_gather_energy(const TraceParams &p, int geo, int D, const GatherEnergyArgs &ea, unsigned slabs, hipStream_t st) {
  const GatherArgs &a = ea.a;
  if (!gather_energy_ok(ea))
    return hipErrorInvalidValue;
  // a list goes with the sums alone and is no longer than the range (its entries index the range)
  if (a.stat ? !a.accSq || (a.list && a.listCount > a.primCount) ||
                   (unsigned long long)(a.chunkFirst + (unsigned long long)a.chunks) * GATHER_CHUNK > a.samples
             : a.list != nullptr)
    return hipErrorInvalidValue;
  // no more waves than slabs, no more than work items; whole blocks of VR_BLOCK / 64 waves once there are that many
  const unsigned long long items = (unsigned long long)a.groups * a.chunks * a.subs;
  const unsigned perBlock = VR_BLOCK / 64;
  unsigned waves = items < slabs ? (unsigned)items : slabs;
  if (waves > perBlock)
    waves -= waves % perBlock;
  if (waves == 0)
    return hipSuccess;
  const dim3 g(waves > perBlock ? waves / perBlock : 1u), b(waves > perBlock ? (unsigned)VR_BLOCK : waves * 64u);
  if (a.stat)
    energy_launch<1>(geo, D, g, b, st, p, ea);
  else
    energy_launch<0>(geo, D, g, b, st, p, ea);
  return hipGetLastError();
}

hipError_t launch_gather_energy_tables(const float *hostTable, float *dst, hipStream_t st) {
  if (!hostTable || !dst)
    return hipErrorInvalidValue;
  GatherEnergyTable t;
  for (unsigned k = 0; k < 3 * GATHER_LAW_MAX; ++k)
    t.v[k] = hostTable[k];
  hipLaunchKernelGGL(gather_energy_put_kernel, dim3(3), dim3(GATHER_LAW_MAX), 0, st, t, dst);
  return hipGetLastError();
}

hipError_t launch_debug_gather_energy_path(const TraceParams &p, int geo, int D, const GatherEnergyArgs &ea, unsigned sample,
                                           unsigned maxVertices, float *vertices, float *tail, float *energy4, hipStream_t st) {
  if (!gather_energy_ok(ea) || !ea.a.leafOfOrig || ea.a.stat || !tail || !energy4 || (maxVertices && !vertices))
    return hipErrorInvalidValue;
  // one wave over the one chunk that holds the sample: a range of one primitive, samples 0 .. sample, whole chunks
  GatherEnergyArgs b2 = ea;
  b2.a.primCount = 1u;
  b2.a.groups = 1u;
  b2.a.samples = sample + 1u; // (sample < 2^22: vr_gather_paths.cpp)
  b2.a.chunks = sample / GATHER_CHUNK + 1u;
  b2.a.subs = 1u;
  b2.a.pathSample = sample;
  b2.a.pathMaxVertices = maxVertices;
  b2.a.pathVertices = vertices;
  b2.a.pathTail = tail;
  b2.pathEnergy = energy4;
  const dim3 g(1), b(64);
  if (geo == 0) {
    if (D == 2)
      hipLaunchKernelGGL((gather_energy_kernel<0, 2, 0, true>), g, b, 0, st, p, b2);
    else
      hipLaunchKernelGGL((gather_energy_kernel<0, 3, 0, true>), g, b, 0, st, p, b2);
  } else {
    if (D == 2)
      hipLaunchKernelGGL((gather_energy_kernel<1, 2, 0, true>), g, b, 0, st, p, b2);
    else
      hipLaunchKernelGGL((gather_energy_kernel<1, 3, 0, true>), g, b, 0, st, p, b2);
  }
  return hipGetLastError();
}

} // namespace vr
