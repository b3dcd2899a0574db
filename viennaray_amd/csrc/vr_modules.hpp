// vr_modules.hpp — what a RUN-TIME module is compiled from besides the caller's text (vr_models.cpp writes the
// translation unit; it includes vr_trace.hip with VR_USER_MODULE defined, and vr_trace.hip includes this file):
//   VR_USER_SOURCE_MODULE   a source model: the generator around the caller's sample and its debug twin.  It needs
//                           vr_generate.hpp alone: no particle registry, no trace kernel.
//   otherwise               a particle model: the extended trace kernels with the caller's model compiled in and, for a
//                           stateful model, its generator.
#pragma once
#include "vr_generate.hpp"
#ifndef VR_USER_SOURCE_MODULE
#include "vr_kernel_table.hpp"
#endif

namespace vr {

#ifdef VR_USER_SOURCE_MODULE
// ---------------------------------------------------------------------------
// A SOURCE model registered at RUN TIME (vr_register_source_model, include/viennaray_amd.h): the reference's second
// extension point, Source<NumericType> (raySource.hpp:10-19: getOriginAndDirection(idx, rng), getInitialRayWeight(idx)),
// as device code.  The library writes a translation unit that defines VR_USER_MODULE, VR_USER_SOURCE_MODULE and
// VR_USER_SOURCE_FILE — the caller's text, which defines
//
//   struct VrUserSource {
//     static constexpr bool kHasWeight = ...; // false: every ray starts with weight 1 and the absorbing kernels stay eligible
//     template <int D, class Draw>
//     __device__ static void sample(const SourceCtx &s, unsigned long long idx, Draw &&draw, V3 &org, V3 &dir, float &weight);
//   };
//
// — and includes vr_trace.hip, which as a module is this file: a code object with the generator and its debug twin only, no trace kernel.  draw() is the next
// raw 64-bit output of ray idx's engine (tea3(idx, seed), rng_next): any number of them, lane by lane; canon_f32 / canon_f64
// turn one into the reference's uniform float / double.  `dir` is used as returned: the model normalises it (vnormalize).
// `weight` is 1 on entry and read only with kHasWeight.  SourceCtx: vr_types.hpp.
//
// The record, its sort bin and the side array are a host-ray apply's (gen_host_kernel): the trace launch is that launch.
// ---------------------------------------------------------------------------
#include VR_USER_SOURCE_FILE
static_assert(VrUserSource::kHasWeight == (VR_USER_SOURCE_HAS_WEIGHT != 0), "kHasWeight differs from the VR_SOURCE_HAS_WEIGHT flag given at registration");

template <int D>
__device__ __forceinline__ void user_source_sample(const SourceCtx &sc, unsigned long long idx, Rng &rng, V3 &o, V3 &d, float &w) {
  unsigned t2 = 0; // (a full state built HERE is the generator's own: the tracer rebuilds it from k and counts it then)
  o = mk(0.f, 0.f, 0.f);
  d = mk(0.f, 0.f, 0.f);
  w = 1.f;
  VrUserSource::template sample<D>(sc, idx, [&]() { return rng_next(rng, t2); }, o, d, w);
  if (!VrUserSource::kHasWeight)
    w = 1.f;
}

template <int D, bool KEEP> __global__ __launch_bounds__(VR_BLOCK) void gen_user_source_kernel(const TraceParams p, const SourceCtx sc) {
  const unsigned tid = threadIdx.x;
  const unsigned gwave = (blockIdx.x * VR_BLOCK + tid) >> 6; // physical wave of this (bounded) grid
  u64 *scratchLane = p.rngScratch + (size_t)gwave * (312u * 64u) + (tid & 63u);
  for (unsigned i = blockIdx.x * VR_BLOCK + tid; i < p.batchCount; i += gridDim.x * VR_BLOCK) {
    const unsigned long long idx = p.idxList ? p.idxList[i] : p.batchFirst + i;
    Rng rng;
    rng_init(rng, tea3((unsigned)idx, p.seed), scratchLane);
    V3 o, d;
    float w;
    user_source_sample<D>(sc, idx, rng, o, d, w);
    gen_store<D, KEEP>(p, i, o, d, rng.k, rng.lo, rng.hi); // (k >= 156: the trace kernel rebuilds the full state from the seed and skips k outputs)
    // the start weight goes where gen_surface_kernel puts it: the batch's buffer, addressed by GLOBAL ray index
    if (VrUserSource::kHasWeight && p.hostWeights)
      const_cast<float *>(p.hostWeights)[p.batchFirst + i] = w;
  }
}

// vr_debug_user_source_sample: what the generator's sample gives for the p.batchCount ray indices p.idxList[]
template <int D>
__global__ __launch_bounds__(VR_BLOCK) void debug_user_source_kernel(const TraceParams p, const SourceCtx sc, float *org, float *dir,
                                                                     float *weight, unsigned *draws) {
  const unsigned tid = threadIdx.x;
  const unsigned gwave = (blockIdx.x * VR_BLOCK + tid) >> 6;
  u64 *scratchLane = p.rngScratch + (size_t)gwave * (312u * 64u) + (tid & 63u);
  for (unsigned i = blockIdx.x * VR_BLOCK + tid; i < p.batchCount; i += gridDim.x * VR_BLOCK) {
    const unsigned long long idx = p.idxList[i];
    Rng rng;
    rng_init(rng, tea3((unsigned)idx, p.seed), scratchLane);
    V3 o, d;
    float w;
    user_source_sample<D>(sc, idx, rng, o, d, w);
    org[3 * (size_t)i] = o.x;
    org[3 * (size_t)i + 1] = o.y;
    org[3 * (size_t)i + 2] = o.z;
    dir[3 * (size_t)i] = d.x;
    dir[3 * (size_t)i + 1] = d.y;
    dir[3 * (size_t)i + 2] = d.z;
    weight[i] = w;
    draws[i] = rng.k;
  }
}
template __global__ void gen_user_source_kernel<2, false>(const TraceParams, const SourceCtx);
template __global__ void gen_user_source_kernel<2, true>(const TraceParams, const SourceCtx);
template __global__ void gen_user_source_kernel<3, false>(const TraceParams, const SourceCtx);
template __global__ void gen_user_source_kernel<3, true>(const TraceParams, const SourceCtx);
template __global__ void debug_user_source_kernel<2>(const TraceParams, const SourceCtx, float *, float *, float *, unsigned *);
template __global__ void debug_user_source_kernel<3>(const TraceParams, const SourceCtx, float *, float *, float *, unsigned *);

#else // a particle module
// ---------------------------------------------------------------------------
// A particle model registered at RUN TIME (vr_register_particle_model, include/viennaray_amd.h): the library writes a
// translation unit that defines VR_USER_MODEL_FILE (the caller's model source: `struct VrUserModel`, appended to the
// registry in vr_particles.hpp) and includes vr_trace.hip, which as a module is this file; `hipcc --genco` turns it into a code object holding the
// extended trace kernels with that model compiled in.  The host finds them by their mangled names.
// ---------------------------------------------------------------------------
static_assert(VrUserModel::kNumData >= 1 && VrUserModel::kNumData <= VR_MAX_LABELS, "a model has 1 .. VR_MAX_LABELS data labels");
static_assert(VrUserModel::kNumData == VR_USER_NUM_DATA, "kNumData differs from the count given at registration");
#ifndef VR_USER_NUM_STATE
#define VR_USER_NUM_STATE 0
#endif
static_assert(VrUserModel::kStateWords >= 0 && VrUserModel::kStateWords <= VR_MAX_STATE_WORDS, "a model has 0 .. 4 state words (kStateWords)");
static_assert(VrUserModel::kStateWords == VR_USER_NUM_STATE, "kStateWords differs from the numState given at registration");
static_assert(VrUserModel::kStateWords == 0 || VrUserModel::kNeedsFull, "a stateful model (kStateWords > 0) needs kNeedsFull = true");
static_assert(VrUserModel::kLogRows >= 0 && VrUserModel::kLogRows <= VR_LOG_MAX_ROWS, "a model logs into 0 .. 16 rows of the data log (kLogRows)");
static_assert(VrUserModel::kLogRows == 0 || VrUserModel::kStateWords > 0, "log_data (kLogRows > 0) logs the state init left: it needs a stateful model (kStateWords > 0)");
// what the host asks the loaded module (vr_register_particle_model): the rows its log_data hook writes
extern "C" __device__ __attribute__((used)) const int vr_user_log_rows = VrUserModel::kLogRows;
// (VR_USER_FLUX_STATS: the module's twin with flux statistics compiled in, built when a statistics-on apply first needs it)
#ifndef VR_USER_FLUX_STATS
#define VR_USER_FLUX_STATS 0
#endif
static_assert(!VR_USER_FLUX_STATS || VrUserModel::kNumData <= VR_MAX_LABELS - VR_STAT_PLANES, "flux statistics take two of a particle's planes");
// the module's one particle id, and its trace kernels: what the catalogue (trace_kernel_exists, vr_types.hpp) lists for
// KERNELS_MODULE under that id — the table is what instantiates them (vr_models.cpp, find_trace_kernels, asks the same predicate)
constexpr int VR_USER_P = VR_USER_FLUX_STATS ? (VrUserModel::kNeedsFull ? P_EXT_FULL_STATS : P_EXT_STATS) : (VrUserModel::kNeedsFull ? P_EXT_FULL : P_EXT);
template struct TraceKernelTable<VR_USER_P, VR_USER_P>;

// The generator of a STATEFUL model (SourceRandom, plain or with a primary direction): the model's init (initNew,
// rayTraceKernel.hpp:131-133) draws first, then the source sample from the same engine (the streaming generator of
// gen_basis_kernel: the draw count varies), then the record with the true draw count — always with the side array
// (TraceParams::recExtra) — and the ray's state at the same index (TraceParams::rayState).
//
// A model with a log_data hook (kLogRows > 0; the reference's logData, called right after initNew, and the per-thread DataLog
// merged into Trace::getDataLog(), rayTraceKernel.hpp:131-133, 345) adds to the apply's data log here: int64 fixed-point
// sums (value * 2^24), so the result does not depend on the grid, the batch split or the rank count.  A block sums into
// a private copy of the log in LDS (VR_LOG_LDS_ENTRIES) and adds its non-zero entries to HBM once, when its loop ends;
// a log beyond that budget (or VR_LOG_FLAGS bit 0) adds to HBM directly.  Overflow is detected by the adds themselves: every
// add returns the sum it produced.  One add is at most 2^39, so a sum cannot pass from below 2^63 to beyond 2^64 without
// one add seeing its top bit: an LDS sum with that bit raises the flag (the total is then out of range for any rank count),
// and every add to HBM checks the carry and the bound 2^(63 - headroom) of the new total — sums only grow, so the add that
// comes last sees the final value.  Without a shape (the frame's VR_F_LOG_* = 0) nothing of this runs.
template <int D, class M = VrUserModel> __global__ __launch_bounds__(VR_BLOCK) void gen_state_kernel(const TraceParams p) {
  if constexpr (M::kStateWords > 0) {
    const unsigned tid = threadIdx.x;
    const unsigned gwave = (blockIdx.x * VR_BLOCK + tid) >> 6; // physical wave of this (bounded) grid
    u64 *scratchLane = p.rngScratch + (size_t)gwave * (312u * 64u) + (tid & 63u);
    const ModelCtx mctx = model_ctx(p);
    constexpr bool LOG = M::kLogRows > 0;
    __shared__ u64 logS[LOG ? VR_LOG_LDS_ENTRIES : 1];
    __shared__ unsigned logOffS[LOG ? VR_LOG_MAX_ROWS + 1 : 1];
    u64 *logG = nullptr, *logCtl = nullptr;
    unsigned logRows = 0, logShift = 63, logDropped = 0;
    bool logLds = false, logOverflow = false;
    if constexpr (LOG) {
      logG = reinterpret_cast<u64 *>(frame_addr(p.wallTable, VR_F_LOG_LO));
      if (logG) {
        logCtl = reinterpret_cast<u64 *>(frame_addr(p.wallTable, VR_F_LOGCTL_LO));
        logRows = min((unsigned)logCtl[VR_LOG_ROWS], (unsigned)VR_LOG_MAX_ROWS);
        logShift = 63u - (unsigned)logCtl[VR_LOG_HEADROOM];
        if (tid <= logRows)
          logOffS[tid] = (unsigned)logCtl[VR_LOG_OFFSETS + tid];
        const unsigned total = (unsigned)logCtl[VR_LOG_OFFSETS + logRows];
        logLds = total <= VR_LOG_LDS_ENTRIES && !(logCtl[VR_LOG_FLAGS] & 1ull);
        if (logLds)
          for (unsigned e = tid; e < total; e += VR_BLOCK)
            logS[e] = 0ull;
        __syncthreads();
      }
    }
    for (unsigned i = blockIdx.x * VR_BLOCK + tid; i < p.batchCount; i += gridDim.x * VR_BLOCK) {
      const unsigned long long idx = p.idxList ? p.idxList[i] : p.batchFirst + i;
      Rng rng;
      rng_init(rng, tea3((unsigned)idx, p.seed), scratchLane);
      unsigned t2 = 0;
      RayState s;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        s.v[k] = 0.f;
      M::init(mctx, s, rng, t2);
      if constexpr (LOG) {
        if (logG) {
          const RayState &born = s;
          M::log_data(mctx, born, [&](int row, int bin, float value) {
            bool ok = (unsigned)row < logRows && value >= 0.f && value <= VR_LOG_MAX_VALUE; // (a NaN fails both)
            unsigned e = 0;
            if (ok) {
              e = logOffS[row] + (unsigned)bin;
              ok = (unsigned)bin < logOffS[row + 1] - logOffS[row];
            }
            if (!ok) {
              ++logDropped;
              return;
            }
            const u64 q = (u64)((double)value * VR_LOG_SCALE + 0.5);
            if (logLds)
              logOverflow = logOverflow || ((atomicAdd(&logS[e], q) + q) >> 63) != 0ull;
            else
              logOverflow = logOverflow || ((atomicAdd(&logG[e], q) + q) >> logShift) != 0ull;
          });
        }
      }
      V3 o, d;
      source_sample<D>(p, [&]() { return rng_next(rng, t2); }, o, d);
      gen_store<D, true>(p, i, o, d, rng.k, rng.lo, rng.hi); // (k >= 156: the trace kernel rebuilds tier 2 from the seed)
      reinterpret_cast<float4 *>(frame_addr(p.wallTable, VR_F_STATE_LO))[i] = make_float4(s.v[0], s.v[1], s.v[2], s.v[3]);
    }
    if constexpr (LOG) {
      if (logG) {
        if (logLds) {
          __syncthreads();
          for (unsigned e = tid; e < logOffS[logRows]; e += VR_BLOCK) {
            const u64 v = logS[e];
            if (v) {
              const u64 now = atomicAdd(&logG[e], v) + v;
              logOverflow = logOverflow || now < v || (now >> logShift) != 0ull;
            }
          }
        }
        if (logOverflow)
          logCtl[VR_LOG_OVERFLOW] = 1ull;
        if (logDropped)
          atomicAdd(&logCtl[VR_LOG_DROPPED], (u64)logDropped);
      }
    }
  }
}
template __global__ void gen_state_kernel<2>(const TraceParams);
template __global__ void gen_state_kernel<3>(const TraceParams);
#endif // VR_USER_SOURCE_MODULE

} // namespace vr
