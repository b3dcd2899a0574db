// vr_gather.hip — per-primitive direct flux by rays cast FROM the surface (vr_gather_flux_device; include/viennaray_amd.h
// has the definition, vr_gather.hpp the arithmetic of a sample, vr_gather_flux.cpp the host side).  A translation unit of
// its own, like vr_cast.hip: nothing an apply() runs is in it.
//
//   gather_samples_kernel<GEO, D>  a persistent grid, laid out as cast_rays_kernel: every wave owns one slab of the walk's
//                                  global stack and its lanes' columns of the block's LDS stack for its whole life; the
//                                  launcher never starts more waves than there are slabs or work items.
//                                  With REC it records the link table of vr_radiosity_links_device instead of
//                                  reading an emission table: one text for what a sample is.
//                                  With PATH it follows a sample through its reflections (vr_gather_paths_device,
//                                  vr_gather_paths.cpp): a front-side hit keeps the lane in the segment loop.
//                                  With PATH == 2 it writes ONE path vertex by vertex (vr_debug_gather_path).
//                                  With PATH == 3 the path is weighed by up to three angular laws staged in LDS
//                                  (vr_gather_angular*, vr_gather_angular.cpp); PATH == 2 takes them at run time.
//                                  With STAT it sums a range of chunks for a list of primitives and carries the sum of
//                                  the squared weights beside the sum (vr_gather_sums_device, vr_gather_adaptive_device;
//                                  vr_gather_adaptive.cpp).
//   gather_finish_kernel           int64 sums -> floats.
//   gather_laws_put_kernel         the angular laws of a call, from the launch arguments into device memory.
//   gather_decide_kernel           one round's verdict of the adaptive gather: outputs of the converged primitives, the
//                                  others compacted in order into the next list.
//   debug_gather_samples_kernel    the origin, the normal and a run of sample directions of ONE primitive
//                                  (vr_debug_gather_samples): the device functions the first kernel uses.
//
// A work item is (a group of 64 primitives) x (one chunk of 64 samples); lane = primitive.  Over the whole scene the
// groups follow the PACKED (Morton) order, so a wave's origins are neighbours; over a sub-range they follow the caller's
// ids through leafOfOrig.  The lane seeds its chunk's engine once — mt_first_outputs<2>, then the two streaming cursors of
// vr_rng.hpp: 128 outputs, inside the streaming tier, no engine state anywhere — and loops over the chunk's samples; the
// wave votes in pair_walk_lanes as in vr_cast.hip, a lane whose sample has ended (or is not walked at all) taking part
// with part = false.  The lane's int64 sum of the chunk stays in registers and goes to the primitive's accumulator with
// one 64-bit vector atomic.  Integer sums: the result has the same bits for any mapping, grid or split of the range.
// Where (groups x chunks) would leave waves idle — a scene of a few ten thousand primitives at K = 64 — the host cuts
// every chunk into a.subs runs of 64 / a.subs samples, work items of their own: such a lane seeds the chunk's engine,
// steps over the draws of the samples before its run (two streaming steps per draw) and walks its run alone.
#include <hip/hip_runtime.h>

#include "vr_cast.hpp"
#include "vr_gather.hpp"
#include "vr_gather_device.hpp"
#include "vr_kernels.hpp"
#include "vr_radiosity.hpp"
#include "vr_trace_kernel.hpp"

namespace vr {

// The step of a path (vr_gather_paths) at a geometry hit: true when the path goes on — from the hit point along the new
// direction, T, c = u . rayDirection and the bounce count updated — false when it ends there, `end` saying how.  hitPos:
// the leaf position of the primitive hit, nj: the normal the tracer tests its side against; startPrim, sample: what the
// counter draw of a DIFFUSE vertex is keyed by.  The kernel and vr_debug_gather_path both step through here.
// PATH >= 2 with a reflectivity law (lawS: the block's staged laws; a.lawCount: wave-uniform): T takes a second multiply,
// by R at mu = n_j . (the direction the path leaves along), and a T of 0 ends the path there as one of rho 0 does
template <int GEO, int D, int PATH = 1>
__device__ __forceinline__ bool gather_bounce(const float4 *__restrict__ prims, const GatherArgs &a, const GatherFrame &frame,
                                              unsigned hitPos, unsigned startPrim, unsigned sample, const V3 &hitPoint, V3 &org,
                                              V3 &rayDirection, V3 &dir, float &T, float &c, unsigned &bounces, int &end, V3 &nj,
                                              [[maybe_unused]] const float *lawS = nullptr) {
  nj = gather_hit_normal<GEO>(prims, hitPos);
  if (!(vdot(dir, nj) < 0.f)) {
    end = GATHER_END_BACK;
    return false;
  }
  if (bounces >= a.maxBounces) {
    end = GATHER_END_BOUNCES;
    return false;
  }
  float rho = a.rho;
  if (a.rhoLeaf)
    rho = a.rhoLeaf[hitPos]; // (hitPos < numPrims: a leaf position the walk returned)
  T = gather_path_throughput(T, rho);
  if (T == 0.f) {
    end = GATHER_END_ABSORBED;
    return false;
  }
  V3 leaving;
  if (a.reflection == GATHER_REFLECT_SPECULAR) // (wave-uniform)
    leaving = reflect_specular(rayDirection, nj);
  else
    leaving = v3(gather_path_diffuse(D, a.seed, startPrim, sample, bounces, GVec{nj.x, nj.y, nj.z}));
  if constexpr (PATH >= 2) {
    if (a.lawCount[GATHER_LAW_REFLECTIVITY]) { // (wave-uniform)
      T = gather_path_throughput_law(T, lawS + GATHER_LAW_REFLECTIVITY * GATHER_LAW_MAX, a.lawCount[GATHER_LAW_REFLECTIVITY],
                                     vdot(nj, leaving));
      if (T == 0.f) {
        end = GATHER_END_ABSORBED;
        return false;
      }
    }
  }
  rayDirection = leaving;
  dir = project_dir<D>(rayDirection);
  org = hitPoint; // (org + dir * t: the tracer's restart)
  c = gather_c(GVec{rayDirection.x, rayDirection.y, rayDirection.z}, frame);
  ++bounces;
  end = GATHER_END_FRONT;
  return true;
}

// vertex v of the path vr_debug_gather_path records: a row of GATHER_PATH_ROW floats, if the caller's table has room for it
__device__ __forceinline__ void gather_path_put(const GatherArgs &a, unsigned v, unsigned id, const V3 &pt, const V3 &in, const V3 &n,
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

// REC: the link recording of vr_radiosity_links_device (vr_radiosity.hpp has the table's index).  The same samples and
// walks; every walked sample stores one int32 — the leaf position of a front-side hit, RADIOSITY_NO_LINK for anything
// else — and only the direct weights are summed, into acc[leaf position].  Whole scene, NORMAL mode, no emission table
// PATH: the paths of vr_gather_paths_device.  The same samples and walks; a front-side hit does not end the sample but
// reflects it on (gather_bounce), the lane staying active with its new origin, rayDirection, dir, T and c, until the path
// reaches the source plane or one of its other ends.  The cast state is the path's: the walls passed count over all of it.
// PATH == 2 is vr_debug_gather_path: a range of ONE primitive, of whose samples lane 0 walks a.pathSample alone and
// writes its vertices (gather_path_put) and the path's tail — the same loop, not a second one
// STAT: the sums of vr_gather_sums_device / vr_gather_adaptive_device (REC false, PATH 0 or 1).  The same samples and
// walks; the item's chunk is a.chunkFirst + chunk, the lane's primitive comes from a.list where there is one, and the
// lane carries a second int64, the sum of gather_q2, to a.accSq
template <int GEO, int D, bool REC, int PATH = 0, int STAT = 0>
__global__ __launch_bounds__(VR_BLOCK) void gather_samples_kernel(const TraceParams p, const GatherArgs a) {
  __shared__ float wallS[VR_WALL_TABLE];
  __shared__ unsigned stackS[VR_STACK_LDS * VR_BLOCK]; // [entry][thread of the block]
  for (unsigned k = threadIdx.x; k < VR_WALL_TABLE; k += blockDim.x)
    wallS[k] = p.wallTable[k];
  [[maybe_unused]] const float *lawS = nullptr; // (PATH >= 2) the three laws, staged beside the wall table
  if constexpr (PATH >= 2) {
    __shared__ float lawBuf[3 * GATHER_LAW_MAX];
    if (a.laws) // (block-uniform; absent laws are never read: a.lawCount says which are there)
      for (unsigned k = threadIdx.x; k < 3 * GATHER_LAW_MAX; k += blockDim.x)
        lawBuf[k] = a.laws[k];
    lawS = lawBuf;
  }
  __syncthreads(); // (the only block-wide point: from here on the waves run on their own)
  const unsigned lane = threadIdx.x & 63u;
  const unsigned wavesPerBlock = blockDim.x >> 6;
  const unsigned wave = blockIdx.x * wavesPerBlock + (threadIdx.x >> 6); // < waves <= the slabs of p.walkStack (launch_gather_samples)
  const unsigned waves = gridDim.x * wavesPerBlock;
  unsigned *const stackL = stackS + threadIdx.x;
  unsigned *const stackG = p.walkStack + (size_t)wave * (VR_STACK_GLOBAL * 64u) + lane;
  const uint4 *__restrict__ pnodes = reinterpret_cast<const uint4 *>(p.pnodes);
  const float4 *__restrict__ prims = reinterpret_cast<const float4 *>(p.prims);
  const GatherFrame frame{p.rayDir, p.firstDir, p.secondDir, -p.posNeg};
  const bool haveEmission = !REC && a.emission != nullptr;
#ifdef VR_DIAG
  unsigned long long phaseDummy[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tLast = 0ull;
  unsigned long long *const phaseT = phaseDummy;
#endif
  VR_DIAG_DECL
  const unsigned run = GATHER_CHUNK / a.subs; // samples of a work item: a.subs runs per chunk
  const u64 perGroup = (u64)a.chunks * a.subs, items = (u64)a.groups * perGroup;
  for (u64 it = wave; it < items; it += waves) {
    const unsigned sub = (unsigned)(it % a.subs), chunk = (STAT ? a.chunkFirst : 0u) + (unsigned)((it / a.subs) % a.chunks);
    if constexpr (PATH == 2) {
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
      const GVec w0 = gather_direction(a.mode, D, r1, r2, m, a.cosinePower, frame);
      const float c = gather_c(w0, frame), mDotW = gather_dot(m, w0);
      V3 org = v3(o), rayDirection = v3(w0), dir = project_dir<D>(rayDirection);
      // (a SOURCE sample facing away from the primitive weighs 0 whatever it meets: not walked)
      bool active = valid && !(a.mode == GATHER_SOURCE && !(mDotW > 0.f));
      if constexpr (PATH == 2)
        active = active && lane == 0u && chunk * GATHER_CHUNK + j == a.pathSample;
      const bool walked = active;
      CastState s;
      cast_begin(s);
      bool ignored = false;
      unsigned hitPos = 0u;
      [[maybe_unused]] float T = 1.f, cEnd = c; // (PATH) the throughput, and u . omega of the direction the path goes along
      [[maybe_unused]] unsigned bounces = 0u;
      [[maybe_unused]] unsigned pathCount = 1u; // (PATH == 2) vertices so far: vertex 0 is the primitive itself
      [[maybe_unused]] int pathEnd = GATHER_END_MISS;
      [[maybe_unused]] float pathWeight = 0.f; // (PATH == 2) the one sample's unquantised weight
      if constexpr (PATH == 2) {
        if (walked)
          gather_path_put(a, 0u, orig, org, mk(__int_as_float(0x7FC00000), __int_as_float(0x7FC00000), __int_as_float(0x7FC00000)),
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
          if constexpr (PATH) // (one wave-iteration per round of segments, one lane-iteration per segment walked in it)
            DIAG(0);
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
            if constexpr (PATH) {
              if (s.prim >= 0) {
                int end;
                V3 nj;
                [[maybe_unused]] const V3 arriving = rayDirection;
                active = gather_bounce<GEO, D, PATH>(prims, a, frame, hitPos, orig, chunk * GATHER_CHUNK + j, hitPoint, org,
                                                     rayDirection, dir, T, cEnd, bounces, end, nj, lawS);
                if constexpr (PATH == 2) {
                  const float QNAN = __int_as_float(0x7FC00000);
                  gather_path_put(a, pathCount, (unsigned)s.prim, hitPoint, arriving, nj, active ? rayDirection : mk(QNAN, QNAN, QNAN));
                  ++pathCount;
                  pathEnd = end;
                }
              }
            }
          }
        }
      }
      if constexpr (PATH) {
        // (a path that ended on a primitive weighs 0 like one stopped on a wall; vr_debug_gather_path tells the ends apart)
        if (walked) {
          const int tailEnd = s.prim == CAST_MISS ? (ignored ? GATHER_END_IGNORED : GATHER_END_MISS) : GATHER_END_WALL;
          float w;
          if constexpr (PATH >= 2) // (a.lawCount: wave-uniform; with none of the three this is gather_path_weight)
            w = gather_path_weight_laws(tailEnd, a.g, a.cosinePower, cEnd, T,
                                        a.lawCount[GATHER_LAW_SOURCE] ? lawS + GATHER_LAW_SOURCE * GATHER_LAW_MAX : nullptr,
                                        a.lawCount[GATHER_LAW_SOURCE], a.gL,
                                        a.lawCount[GATHER_LAW_YIELD] ? lawS + GATHER_LAW_YIELD * GATHER_LAW_MAX : nullptr,
                                        a.lawCount[GATHER_LAW_YIELD], mDotW);
          else
            w = gather_path_weight(tailEnd, a.g, a.cosinePower, cEnd, T);
          if constexpr (PATH == 2)
            pathWeight = w;
          sum += gather_q(w, a.wmax);
          if constexpr (STAT)
            sumSq += gather_q2(w, a.wmax);
        }
        if constexpr (PATH == 2) {
          if (walked) { // (lane 0, the one sample)
            const int end = s.prim >= 0 ? pathEnd : s.prim == CAST_MISS ? (ignored ? GATHER_END_IGNORED : GATHER_END_MISS) : GATHER_END_WALL;
            a.pathTail[0] = __uint_as_float(pathCount);
            a.pathTail[1] = __uint_as_float((unsigned)end);
            a.pathTail[2] = rayDirection.x, a.pathTail[3] = rayDirection.y, a.pathTail[4] = rayDirection.z;
            a.pathTail[5] = T;
            a.pathTail[6] = pathWeight; // (0 for a path that ended on a primitive: the tail's rule)
          }
        }
      } else if (walked) {
        int end = s.prim == CAST_MISS ? (ignored ? GATHER_END_IGNORED : GATHER_END_MISS) : GATHER_END_WALL;
        float emission = 0.f;
        if (s.prim >= 0) {
          end = vdot(dir, gather_hit_normal<GEO>(prims, hitPos)) < 0.f ? GATHER_END_FRONT : GATHER_END_BACK;
          if (end == GATHER_END_FRONT && haveEmission)
            emission = a.emission[(unsigned)s.prim]; // (the one load of the emission table: at a front-side hit)
        }
        const float w = gather_weight(end, a.mode, a.g, a.cosinePower, c, mDotW, haveEmission, emission);
        sum += gather_q(w, a.wmax);
        if constexpr (STAT)
          sumSq += gather_q2(w, a.wmax);
        if (REC) // (t < a.primCount <= a.linkSlots, the sample < a.samples: inside the table's linkSlots x samples entries)
          a.links[radiosity_link_index(a.linkSlots, (unsigned)t, chunk * GATHER_CHUNK + j)] =
              end == GATHER_END_FRONT ? (int)hitPos : RADIOSITY_NO_LINK;
      }
      if (j + 1u < jEnd) { // outputs 2 (j + 1) and 2 (j + 1) + 1
        r1 = gather_canon(gather_draw(k, lo, hi));
        r2 = gather_canon(gather_draw(k, lo, hi));
      }
    }
    if (valid && sum != 0)
      atomicAdd(a.acc + (REC ? (unsigned)t : orig - a.primFirst), (unsigned long long)sum);
    if constexpr (STAT) {
      if (valid && sumSq != 0)
        atomicAdd(a.accSq + (orig - a.primFirst), (unsigned long long)sumSq);
    }
  }
#ifdef VR_DIAG
  if constexpr (PATH) { // the rounds of segments and the segments walked in them: vr_gather_paths.cpp prints the two sums
    const unsigned long long sw = wave_sum(diagW[0]), sl = wave_sum(diagL[0]);
    if (lane == 0u && sl) {
      atomicAdd(&p.counters[C_DIAG], sw);
      atomicAdd(&p.counters[C_DIAG + 1], sl);
    }
  }
#endif
}

__global__ void gather_finish_kernel(const unsigned long long *acc, unsigned n, unsigned samples, float *out) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n)
    out[i] = gather_result((long long)acc[i], samples);
}

// the three angular laws of a call from the launch's own arguments (3 KiB of them) into the table the PATH >= 2 kernels
// stage: no host buffer has to outlive the call, and the write is ordered on the stream like any kernel
struct GatherLawTable {
  float v[3 * GATHER_LAW_MAX];
};
__global__ void gather_laws_put_kernel(const GatherLawTable t, float *dst) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 3 * GATHER_LAW_MAX)
    dst[i] = t.v[i];
}

// One round's verdict of vr_gather_adaptive_device: one thread per entry of the current list, a block per
// GATHER_DECIDE_BLOCK entries.  The next list keeps the order of the current one, so a wave's origins stay neighbours:
// a lane's place is (kept entries of the blocks before) + (of the block's waves before) + (of the wave's lanes before) —
// wave ballots and a block prefix, no atomic append.  WRITE false: the block's count alone, for a list of more than one
// block; WRITE true: the outputs and the next list, the block's base summed from those counts (none for block 0)
template <bool WRITE> __global__ __launch_bounds__(GATHER_DECIDE_BLOCK) void gather_decide_kernel(const GatherDecideArgs d) {
  __shared__ unsigned waveCount[GATHER_DECIDE_BLOCK / 64];
  __shared__ unsigned red[GATHER_DECIDE_BLOCK];
  const unsigned e = blockIdx.x * GATHER_DECIDE_BLOCK + threadIdx.x; // (count <= 2^32 - 1: a primitive range)
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const bool have = e < d.count;
  unsigned entry = 0u, idx = 0u;
  long long S1 = 0, S2 = 0;
  bool keep = false;
  if (have) {
    entry = d.list ? d.list[e] : e;
    idx = d.origWords ? d.origWords[(size_t)entry * d.origStride + d.origOffset] : entry; // < the range's primCount
    S1 = (long long)d.acc[idx];
    S2 = (long long)d.accSq[idx];
    keep = !gather_converged(S1, S2, d.samples, d.rel, d.abs);
  }
  const unsigned long long mask = ballot64(keep);
  if (lane == 0u)
    waveCount[wave] = (unsigned)__popcll(mask);
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
    if (have) {
      if (!keep || d.last) {
        d.flux[idx] = gather_result(S1, d.samples);
        if (d.stdErr)
          d.stdErr[idx] = (float)sqrt(gather_stderr2(S1, S2, d.samples));
        if (d.samplesUsed)
          d.samplesUsed[idx] = d.samples;
      }
      if (keep) // (base + before + the lanes before < the kept entries of the whole list <= count: inside `next`)
        d.next[base + before + (unsigned)__popcll(mask & ((1ull << lane) - 1ull))] = entry;
    }
    if (blockIdx.x == gridDim.x - 1u && threadIdx.x == 0u)
      *d.word = base + total;
  }
}

// one thread per sample first + k of primitive a.primFirst; thread 0 also writes the origin and the normal
template <int GEO, int D>
__global__ void debug_gather_samples_kernel(const TraceParams p, const GatherArgs a, unsigned first, unsigned count, float *origin3,
                                            float *normal3, float *directions3) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count && i != 0u)
    return;
  GVec o, m;
  unsigned orig;
  gather_primitive<GEO>(reinterpret_cast<const float4 *>(p.prims), a.leafOfOrig[a.primFirst], o, m, orig);
  if (i == 0u) {
    origin3[0] = o.x, origin3[1] = o.y, origin3[2] = o.z;
    normal3[0] = m.x, normal3[1] = m.y, normal3[2] = m.z;
  }
  if (i >= count)
    return;
  const u64 sample = (u64)first + i;
  const unsigned chunk = (unsigned)(sample / GATHER_CHUNK), j = (unsigned)(sample % GATHER_CHUNK);
  u64 out[2], lo, hi;
  mt_first_outputs<2>(gather_chunk_seed(orig, a.seed, chunk), out, lo, hi);
  unsigned k = 2u;
  float r1 = gather_canon(out[0]), r2 = gather_canon(out[1]);
  for (unsigned s = 0; s < j; ++s) {
    r1 = gather_canon(gather_draw(k, lo, hi));
    r2 = gather_canon(gather_draw(k, lo, hi));
  }
  const GatherFrame frame{p.rayDir, p.firstDir, p.secondDir, -p.posNeg};
  const GVec w = gather_direction(a.mode, D, r1, r2, m, a.cosinePower, frame);
  directions3[3 * (size_t)i] = w.x, directions3[3 * (size_t)i + 1] = w.y, directions3[3 * (size_t)i + 2] = w.z;
}

// laws go with paths alone, no law has more entries than its place in the table holds, and there is at least one
static bool gather_laws_ok(const GatherArgs &a) {
  const uint32_t *n = a.lawCount;
  if (!a.laws)
    return n[0] == 0 && n[1] == 0 && n[2] == 0;
  for (int w = 0; w < 3; ++w)
    if (n[w] && !gather_law_count_ok(n[w]))
      return false;
  return a.paths == 1u && !a.links && (n[0] || n[1] || n[2]);
}

hipError_t launch_gather_samples(const TraceParams &p, int geo, int D, const GatherArgs &a, unsigned slabs, hipStream_t st) {
  // no more waves than slabs, no more than work items; whole blocks of VR_BLOCK / 64 waves once there are that many
  if (a.subs == 0 || a.subs > GATHER_MAX_SUBS || (a.subs & (a.subs - 1u)))
    return hipErrorInvalidValue;
  const unsigned long long items = (unsigned long long)a.groups * a.chunks * a.subs;
  const unsigned perBlock = VR_BLOCK / 64;
  unsigned waves = items < slabs ? (unsigned)items : slabs;
  if (waves > perBlock)
    waves -= waves % perBlock;
  if (waves == 0)
    return hipSuccess;
  if (!gather_laws_ok(a))
    return hipErrorInvalidValue;
  const dim3 g(waves > perBlock ? waves / perBlock : 1u), b(waves > perBlock ? (unsigned)VR_BLOCK : waves * 64u);
  if (a.stat) { // the sums: chunks from a.chunkFirst on, a list of primitives or all of the range, no recording
    if (a.links || !a.accSq || a.paths > 1u || (a.list ? a.listCount > a.primCount : false) ||
        (unsigned long long)(a.chunkFirst + (unsigned long long)a.chunks) * GATHER_CHUNK > a.samples)
      return hipErrorInvalidValue;
    if (a.paths && (a.emission || a.mode != GATHER_NORMAL || a.reflection > GATHER_REFLECT_DIFFUSE || a.maxBounces > GATHER_MAX_BOUNCES))
      return hipErrorInvalidValue;
    if (geo == 0) {
      if (D == 2) {
        if (a.laws)
          hipLaunchKernelGGL((gather_samples_kernel<0, 2, false, 3, 1>), g, b, 0, st, p, a);
        else if (a.paths)
          hipLaunchKernelGGL((gather_samples_kernel<0, 2, false, 1, 1>), g, b, 0, st, p, a);
        else
          hipLaunchKernelGGL((gather_samples_kernel<0, 2, false, 0, 1>), g, b, 0, st, p, a);
      } else {
        if (a.laws)
          hipLaunchKernelGGL((gather_samples_kernel<0, 3, false, 3, 1>), g, b, 0, st, p, a);
        else if (a.paths)
          hipLaunchKernelGGL((gather_samples_kernel<0, 3, false, 1, 1>), g, b, 0, st, p, a);
        else
          hipLaunchKernelGGL((gather_samples_kernel<0, 3, false, 0, 1>), g, b, 0, st, p, a);
      }
    } else {
      if (D == 2) {
        if (a.laws)
          hipLaunchKernelGGL((gather_samples_kernel<1, 2, false, 3, 1>), g, b, 0, st, p, a);
        else if (a.paths)
          hipLaunchKernelGGL((gather_samples_kernel<1, 2, false, 1, 1>), g, b, 0, st, p, a);
        else
          hipLaunchKernelGGL((gather_samples_kernel<1, 2, false, 0, 1>), g, b, 0, st, p, a);
      } else {
        if (a.laws)
          hipLaunchKernelGGL((gather_samples_kernel<1, 3, false, 3, 1>), g, b, 0, st, p, a);
        else if (a.paths)
          hipLaunchKernelGGL((gather_samples_kernel<1, 3, false, 1, 1>), g, b, 0, st, p, a);
        else
          hipLaunchKernelGGL((gather_samples_kernel<1, 3, false, 0, 1>), g, b, 0, st, p, a);
      }
    }
    return hipGetLastError();
  }
  if (a.links) { // the recording: the whole scene in leaf order, NORMAL samples, a table of linkSlots x samples entries
    if (a.paths || a.leafOfOrig || a.emission || a.mode != GATHER_NORMAL || a.primFirst != 0u || a.linkSlots < a.primCount)
      return hipErrorInvalidValue;
    if (geo == 0) {
      if (D == 2)
        hipLaunchKernelGGL((gather_samples_kernel<0, 2, true>), g, b, 0, st, p, a);
      else
        hipLaunchKernelGGL((gather_samples_kernel<0, 3, true>), g, b, 0, st, p, a);
    } else {
      if (D == 2)
        hipLaunchKernelGGL((gather_samples_kernel<1, 2, true>), g, b, 0, st, p, a);
      else
        hipLaunchKernelGGL((gather_samples_kernel<1, 3, true>), g, b, 0, st, p, a);
    }
    return hipGetLastError();
  }
  if (a.paths) { // the paths: NORMAL samples, no emission table
    if (a.emission || a.mode != GATHER_NORMAL || a.reflection > GATHER_REFLECT_DIFFUSE || a.maxBounces > GATHER_MAX_BOUNCES)
      return hipErrorInvalidValue;
    if (a.laws) { // the paths with angular laws
      if (geo == 0) {
        if (D == 2)
          hipLaunchKernelGGL((gather_samples_kernel<0, 2, false, 3>), g, b, 0, st, p, a);
        else
          hipLaunchKernelGGL((gather_samples_kernel<0, 3, false, 3>), g, b, 0, st, p, a);
      } else {
        if (D == 2)
          hipLaunchKernelGGL((gather_samples_kernel<1, 2, false, 3>), g, b, 0, st, p, a);
        else
          hipLaunchKernelGGL((gather_samples_kernel<1, 3, false, 3>), g, b, 0, st, p, a);
      }
      return hipGetLastError();
    }
    if (geo == 0) {
      if (D == 2)
        hipLaunchKernelGGL((gather_samples_kernel<0, 2, false, 1>), g, b, 0, st, p, a);
      else
        hipLaunchKernelGGL((gather_samples_kernel<0, 3, false, 1>), g, b, 0, st, p, a);
    } else {
      if (D == 2)
        hipLaunchKernelGGL((gather_samples_kernel<1, 2, false, 1>), g, b, 0, st, p, a);
      else
        hipLaunchKernelGGL((gather_samples_kernel<1, 3, false, 1>), g, b, 0, st, p, a);
    }
    return hipGetLastError();
  }
  if (geo == 0) {
    if (D == 2)
      hipLaunchKernelGGL((gather_samples_kernel<0, 2, false>), g, b, 0, st, p, a);
    else
      hipLaunchKernelGGL((gather_samples_kernel<0, 3, false>), g, b, 0, st, p, a);
  } else {
    if (D == 2)
      hipLaunchKernelGGL((gather_samples_kernel<1, 2, false>), g, b, 0, st, p, a);
    else
      hipLaunchKernelGGL((gather_samples_kernel<1, 3, false>), g, b, 0, st, p, a);
  }
  return hipGetLastError();
}

hipError_t launch_gather_finish(const unsigned long long *acc, unsigned n, unsigned samples, float *out, hipStream_t st) {
  if (n == 0)
    return hipSuccess;
  hipLaunchKernelGGL(gather_finish_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, acc, n, samples, out);
  return hipGetLastError();
}

hipError_t launch_gather_laws(const float *hostTable, float *dst, hipStream_t st) {
  if (!hostTable || !dst)
    return hipErrorInvalidValue;
  GatherLawTable t;
  for (unsigned k = 0; k < 3 * GATHER_LAW_MAX; ++k)
    t.v[k] = hostTable[k];
  hipLaunchKernelGGL(gather_laws_put_kernel, dim3(3), dim3(GATHER_LAW_MAX), 0, st, t, dst);
  return hipGetLastError();
}

hipError_t launch_gather_decide(const GatherDecideArgs &d, hipStream_t st) {
  if (d.count == 0 || !d.acc || !d.accSq || !d.next || !d.blockCounts || !d.word || !d.flux || d.samples < 2u)
    return hipErrorInvalidValue;
  // one launch where the list fits a block, otherwise the blocks' counts first
  const unsigned blocks = (unsigned)(((unsigned long long)d.count + GATHER_DECIDE_BLOCK - 1u) / GATHER_DECIDE_BLOCK);
  if (blocks > 1u)
    hipLaunchKernelGGL((gather_decide_kernel<false>), dim3(blocks), dim3(GATHER_DECIDE_BLOCK), 0, st, d);
  hipLaunchKernelGGL((gather_decide_kernel<true>), dim3(blocks), dim3(GATHER_DECIDE_BLOCK), 0, st, d);
  return hipGetLastError();
}

hipError_t launch_debug_gather_samples(const TraceParams &p, int geo, int D, const GatherArgs &a, unsigned first, unsigned count,
                                       float *origin3, float *normal3, float *directions3, hipStream_t st) {
  const dim3 g(count ? (count + 63u) / 64u : 1u), b(64); // (count == 0: the origin and the normal alone)
  if (geo == 0) {
    if (D == 2)
      hipLaunchKernelGGL((debug_gather_samples_kernel<0, 2>), g, b, 0, st, p, a, first, count, origin3, normal3, directions3);
    else
      hipLaunchKernelGGL((debug_gather_samples_kernel<0, 3>), g, b, 0, st, p, a, first, count, origin3, normal3, directions3);
  } else {
    if (D == 2)
      hipLaunchKernelGGL((debug_gather_samples_kernel<1, 2>), g, b, 0, st, p, a, first, count, origin3, normal3, directions3);
    else
      hipLaunchKernelGGL((debug_gather_samples_kernel<1, 3>), g, b, 0, st, p, a, first, count, origin3, normal3, directions3);
  }
  return hipGetLastError();
}

hipError_t launch_debug_gather_path(const TraceParams &p, int geo, int D, const GatherArgs &a, unsigned sample, unsigned maxVertices,
                                    float *vertices, float *tail, hipStream_t st) {
  if (!a.paths || !a.leafOfOrig || a.emission || a.links || a.mode != GATHER_NORMAL || a.reflection > GATHER_REFLECT_DIFFUSE ||
      a.maxBounces > GATHER_MAX_BOUNCES || !a.acc || !tail || (maxVertices && !vertices) || !gather_laws_ok(a))
    return hipErrorInvalidValue;
  // one wave over the one chunk that holds the sample: a range of one primitive, samples 0 .. sample, whole chunks
  GatherArgs b2 = a;
  b2.primCount = 1u;
  b2.groups = 1u;
  b2.samples = sample + 1u; // (sample < 2^22: vr_gather_paths.cpp)
  b2.chunks = sample / GATHER_CHUNK + 1u;
  b2.subs = 1u;
  b2.pathSample = sample;
  b2.pathMaxVertices = maxVertices;
  b2.pathVertices = vertices;
  b2.pathTail = tail;
  const dim3 g(1), b(64);
  if (geo == 0) {
    if (D == 2)
      hipLaunchKernelGGL((gather_samples_kernel<0, 2, false, 2>), g, b, 0, st, p, b2);
    else
      hipLaunchKernelGGL((gather_samples_kernel<0, 3, false, 2>), g, b, 0, st, p, b2);
  } else {
    if (D == 2)
      hipLaunchKernelGGL((gather_samples_kernel<1, 2, false, 2>), g, b, 0, st, p, b2);
    else
      hipLaunchKernelGGL((gather_samples_kernel<1, 3, false, 2>), g, b, 0, st, p, b2);
  }
  return hipGetLastError();
}

} // namespace vr
