// vr_generate.hpp — everything a ray generator is made of: the source sampling, the sort keys, the record store, the
// surface sampler and, for the library, its five generators (vr_trace.hip has their table and launcher).
//
// A run-time compiled particle module builds its own generator (gen_state_kernel, vr_modules.hpp) from the source
// sampling and the record store below; a run-time compiled SOURCE module holds a generator alone and reads nothing of
// the tracer but this file.
#pragma once
#include "vr_device.hpp"
#include "vr_types.hpp"
#include "vr_bin_grid.hpp"

namespace vr {

// ---------------------------------------------------------------------------
// source sampling (raySourceRandom.hpp:25-116)
// ---------------------------------------------------------------------------
// `draw()` returns the next raw 64-bit engine output
template <int D, class Draw>
__device__ __forceinline__ void source_sample(const TraceParams &p, Draw &&draw, V3 &org, V3 &dir) {
  // origin draws first (raySourceRandom.hpp:50-68)
  org = mk(0.f, 0.f, 0.f);
  const float r1 = canon_f32(draw());
  setc(org, p.rayDir, p.srcCoord);
  setc(org, p.firstDir, p.lo1 + (p.hi1 - p.lo1) * r1);
  if (D == 2) {
    setc(org, p.secondDir, 0.f);
  } else {
    const float r2 = canon_f32(draw());
    setc(org, p.secondDir, p.lo2 + (p.hi2 - p.lo2) * r2);
  }
  // then the direction draws (raySourceRandom.hpp:70-116)
  if (!p.useBasis) {
    const float d1 = canon_f32(draw());
    const float d2 = canon_f32(draw());
    float ct, st, cp, sp;
    cosine_sample(d1, d2, p.ee, ct, st, cp, sp);
    dir = mk(0.f, 0.f, 0.f);
    setc(dir, p.rayDir, p.posNeg * ct);
    setc(dir, p.firstDir, cp * st);
    setc(dir, p.secondDir, sp * st);
  } else {
    float dr;
    do {
      const float d1 = canon_f32(draw());
      const float d2 = canon_f32(draw());
      float ct, st, cp, sp;
      cosine_sample(d1, d2, p.ee, ct, st, cp, sp);
      const float a = ct, b = cp * st, c = sp * st;
      dir.x = (p.basis[0] * a + p.basis[3] * b) + p.basis[6] * c;
      dir.y = (p.basis[1] * a + p.basis[4] * b) + p.basis[7] * c;
      dir.z = (p.basis[2] * a + p.basis[5] * b) + p.basis[8] * c;
      dr = getc(dir, p.rayDir);
    } while ((p.posNeg < 0.f && dr > 0.f) || (p.posNeg > 0.f && dr < 0.f));
  }
}

__device__ __forceinline__ unsigned part1by1(unsigned v) {
  v &= 0x0000FFFFu;
  v = (v | (v << 8)) & 0x00FF00FFu;
  v = (v | (v << 4)) & 0x0F0F0F0Fu;
  v = (v | (v << 2)) & 0x33333333u;
  v = (v | (v << 1)) & 0x55555555u;
  return v;
}

// Sort key of a ray: the cell in which it crosses the FAR plane of the geometry's
// bounding box (the plane opposite the source), folded back into the domain the
// way the side walls would (periodic wrap / mirror).  For surface-like
// geometry that is where the ray ends up and where the BVH is deepest, so the 64
// rays of a wavefront walk (almost) the same nodes and leaves.  Cells are
// Morton-ordered so consecutive bins are spatial neighbours.  The key only
// orders the work; it has no influence on any result.
// (fold_unit, bin_cell and bin_index: vr_bin_grid.hpp, which the host tests compile too)
template <int D> __device__ __forceinline__ unsigned bin_of(const TraceParams &p, const V3 &org, const V3 &dir) {
  // sort plane: the coordinate on the tracing axis where most first hits are expected
  const float keyCoord = p.keyCoord;
  const float dr = getc(dir, p.rayDir);
  float t = (keyCoord - p.srcCoord) / (fabsf(dr) > 1e-6f ? dr : copysignf(1e-6f, dr == 0.f ? -p.posNeg : dr));
  t = (p.debugFlags & 2u) ? 0.f : (t > 0.f ? t : 0.f); // flag 2: key on the origin instead
  const float u1 = fold_unit((getc(org, p.firstDir) + getc(dir, p.firstDir) * t - p.lo1) * p.invExt1, p.bc0);
  const int c1 = bin_cell(u1, p.binScale1, p.binBias1, p.binT1);
  if (D == 2)
    return (unsigned)c1;
  const float u2 = fold_unit((getc(org, p.secondDir) + getc(dir, p.secondDir) * t - p.lo2) * p.invExt2, p.bc1);
  return bin_index(c1, bin_cell(u2, p.binScale2, p.binBias2, p.binT2), p.binTiles);
}

// Sort key on a scene that is flat WITH RELIEF (TraceParams, round 4): the cell of the ray's PREDICTED first hit — the
// crossing of the plane through the mid height of the coarse relief tile under the previous guess, two look-ups starting
// from the sort plane — so that the rays of a wave meet the surface, not some plane above or below it, in one
// neighbourhood whatever their angles.  A ray whose stretch through the local slab is long (thickness x tan(theta) >
// reliefTravel: a grazing ray) is filed in the coarser LOOSE bins instead (bit 31 of the result): one such ray in a wave
// stretches the packet query's box over dozens of cells.  Like bin_of this only orders the work.
template <int D> __device__ __forceinline__ unsigned bin_of_relief(const TraceParams &p, const V3 &org, const V3 &dir) {
  typedef float F2 __attribute__((ext_vector_type(2)));
  typedef const __attribute__((address_space(1))) F2 *GlobalF2;
  const GlobalF2 coarse = (GlobalF2)p.reliefCoarse;
  const float dr = getc(dir, p.rayDir);
  const float drs = fabsf(dr) > 1e-6f ? dr : copysignf(1e-6f, dr == 0.f ? -p.posNeg : dr);
  // (the key only orders the work: the approximate reciprocal and fused multiply-adds will do, and the look-ups take
  //  the unfolded position, clamped — a ray that crosses a side wall first is sorted a little less well)
  const float inv = __builtin_amdgcn_rcpf(drs);
  const float o1 = getc(org, p.firstDir), d1 = getc(dir, p.firstDir);
  const float o2 = D == 3 ? getc(org, p.secondDir) : 0.f, d2 = D == 3 ? getc(dir, p.secondDir) : 0.f;
  const float a1 = (o1 - p.rcLo1) * p.rcInvT, b1 = d1 * p.rcInvT, a2 = (o2 - p.rcLo2) * p.rcInvT, b2 = d2 * p.rcInvT;
  float t = fmaxf((p.keyCoord - p.srcCoord) * inv, 0.f), thick = 0.f;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    if (it == p.reliefLookups)
      break;
    int cx = (int)__builtin_fmaf(b1, t, a1);
    cx = cx < 0 ? 0 : (cx >= p.rcNx ? p.rcNx - 1 : cx);
    int cy = 0;
    if (D == 3) {
      cy = (int)__builtin_fmaf(b2, t, a2);
      cy = cy < 0 ? 0 : (cy >= p.rcNy ? p.rcNy - 1 : cy);
    }
    const F2 f = coarse[cy * p.rcNx + cx];
    t = fmaxf((f.x - p.srcCoord) * inv, 0.f);
    thick = f.y;
  }
  const float u1 = fold_unit((__builtin_fmaf(d1, t, o1) - p.lo1) * p.invExt1, p.bc0);
  const float sin2 = fmaxf(0.f, 1.f - dr * dr);
  const bool loose = thick * thick * sin2 > p.reliefTravel * p.reliefTravel * (drs * drs) || sin2 > p.reliefTanMax * p.reliefTanMax * (drs * drs);
  // (both sets of bins of a launch with relief packets are PLAIN grids — size_ray_stream, vr_prepare.cpp: the aligned grid
  //  measured slower here — so the key helper gets {T, 0} and the generator reads nothing the parent grid did not have)
  const int T1 = loose ? p.looseT1 : p.binT1, T2 = loose ? p.looseT2 : p.binT2, tiles = loose ? p.looseTiles : p.binTiles;
  const int c1 = bin_cell(u1, (float)T1, 0.f, T1);
  if (D == 2)
    return (unsigned)c1 | (loose ? 0x80000000u : 0u);
  const float u2 = fold_unit((__builtin_fmaf(d2, t, o2) - p.lo2) * p.invExt2, p.bc1);
  const int c2 = bin_cell(u2, (float)T2, 0.f, T2);
  return bin_index(c1, c2, tiles) | (loose ? 0x80000000u : 0u);
}

// ---------------------------------------------------------------------------
// gen_kernel: ray index -> ray record
// ---------------------------------------------------------------------------
// the record of batch ray i in `slot`: both forms of vr_types.hpp
template <bool KEEP>
__device__ __forceinline__ void gen_write(const TraceParams &p, unsigned slot, unsigned i, const V3 &o, const V3 &d, unsigned k,
                                          u64 lo, u64 hi) {
  float4 *rec = reinterpret_cast<float4 *>(p.slotRec) + (size_t)2 * slot;
  if (KEEP) {
    // the compact record (vr_types.hpp) + what the plain generator's rays do not need: origin[rayDir], k, s[k]
    rec[0] = make_float4(getc(o, p.firstDir), getc(o, p.secondDir), d.x, d.y);
    rec[1] = make_float4(d.z, __uint_as_float(i), __uint_as_float((unsigned)(hi & 0xFFFFFFFFull)), __uint_as_float((unsigned)(hi >> 32)));
    reinterpret_cast<float4 *>(const_cast<float *>(p.recExtra))[i] =
        make_float4(getc(o, p.rayDir), __uint_as_float(k), __uint_as_float((unsigned)(lo & 0xFFFFFFFFull)), __uint_as_float((unsigned)(lo >> 32)));
  } else {
    rec[0] = make_float4(o.x, o.y, o.z, d.x);
    rec[1] = make_float4(d.y, d.z, __uint_as_float(i), __uint_as_float(k));
  }
}

// Writes the ray record straight into its sort bin (no separate sort pass): the bin's
// cursor hands out one of p.binCap slots; a ray whose bin is full goes to the
// overflow region, which is traced after the bins.  Returns the record slot.
template <int D, bool KEEP>
__device__ __forceinline__ unsigned gen_store(const TraceParams &p, unsigned i, const V3 &o, const V3 &d, unsigned k,
                                              u64 lo, u64 hi) {
  unsigned slot = i;
  if (p.binCount && !(p.debugFlags & 64u)) { // flag 64: timing experiment, no binning
    const unsigned b = bin_of<D>(p, o, project_dir<D>(d));
    const unsigned pos = atomicAdd(&p.binCount[b], 1u);
    if (pos < p.binCap)
      slot = b * p.binCap + pos;
    else
      slot = p.numBins * p.binCap + atomicAdd(&p.binCount[p.numBins], 1u); // < ovCap by construction
  }
  gen_write<KEEP>(p, slot, i, o, d, k, lo, hi);
  return slot;
}

// Surface source (gpu/raygSource.hpp:65-81, 105-118; gpu/raygTrace.hpp:267-297): global ray idx leaves source point
// j = idx / surfRays from position + unit normal * offset, along a power-1 cosine distribution about the normal (Frisvad
// basis) whatever the particle's source power, with the point's weight.  Two engine outputs, r1 then r2, as in
// gen_grid_kernel.  Consecutive indices share their point: where the whole wave does, the point's seven table words
// come through the scalar cache (one s_load each) instead of 64 identical vector loads.
__device__ __forceinline__ void surface_sample(const TraceParams &p, unsigned idx, V3 &o, V3 &d, float &weight, u64 &lo, u64 &hi) {
  u64 out[2];
  mt_first_outputs<2>(tea3(idx, p.seed), out, lo, hi);
  const float r1 = canon_f32(out[0]), r2 = canon_f32(out[1]);
  const unsigned j = idx / p.surfRays;
  const unsigned j0 = __builtin_amdgcn_readfirstlane(j);
  V3 pos, n;
  if (!ballot64(j != j0)) {
    typedef const float __attribute__((address_space(4))) *ConstF32;
    const ConstF32 sp = (ConstF32)p.surfPos + 3 * (size_t)j0, sn = (ConstF32)p.surfNrm + 3 * (size_t)j0;
    pos = mk(sp[0], sp[1], sp[2]);
    n = mk(sn[0], sn[1], sn[2]);
    weight = ((ConstF32)p.surfWeights)[j0];
  } else {
    const float *sp = p.surfPos + 3 * (size_t)j, *sn = p.surfNrm + 3 * (size_t)j;
    pos = mk(sp[0], sp[1], sp[2]);
    n = mk(sn[0], sn[1], sn[2]);
    weight = p.surfWeights[j];
  }
  vnormalize(n);
  o = mk(pos.x + n.x * p.surfOffset, pos.y + n.y * p.surfOffset, pos.z + n.z * p.surfOffset);
  const float cosT = sqrtf(r2), sinT = sqrtf(fmaxf(0.f, 1.f - cosT * cosT));
  float sinP, cosP;
  glibc_sincosf((float)(3.14159265358979323846 * 2.f * (double)r1), sinP, cosP);
  const float s = copysignf(1.f, n.z), a = -1.f / (s + n.z), b = n.x * n.y * a;
  const V3 t = mk(1.f + s * n.x * n.x * a, s * b, -s * n.x), b2 = mk(b, s + n.y * n.y * a, -n.y);
  const float ct = cosP * sinT, st = sinP * sinT;
  d = mk((n.x * cosT + t.x * ct) + b2.x * st, (n.y * cosT + t.y * ct) + b2.y * st, (n.z * cosT + t.z * ct) + b2.z * st);
  vnormalize(d);
}

#ifndef VR_USER_MODULE
// Fixed number of source draws (no tilted primary direction): the NS engine outputs
// the source sample needs are produced straight into registers by one 156+NS-step pass
// of the seeding recurrence, which also leaves the streaming cursors for the trace kernel.
// The bin cursor's returning atomic is the one long latency of a ray; it is issued as soon as the ray's bin is
// known and its answer is used one loop pass later, after the NEXT ray's seeding chain: the wave computes while
// its own atomic is under way instead of leaving that to the other waves of the SIMD.
// RELIEF: the sort key of bin_of_relief and its second, loose set of bins
template <int D, bool KEEP, bool RELIEF> __global__ __launch_bounds__(VR_BLOCK) void gen_kernel(const TraceParams p) {
  constexpr int NS = D == 3 ? 4 : 3;
  const bool binned = p.binCount && !(p.debugFlags & 64u); // flag 64: timing experiment, no binning
  bool havePrev = false;
  V3 po = mk(0, 0, 0), pd = mk(0, 0, 1);
  unsigned pi = 0, pbin = 0, ppos = 0;
  u64 phi = 0;
  for (unsigned i = blockIdx.x * VR_BLOCK + threadIdx.x;; i += gridDim.x * VR_BLOCK) {
    const bool cur = i < p.batchCount;
    V3 o = mk(0, 0, 0), d = mk(0, 0, 1);
    u64 lo = 0, hi = 0;
    unsigned b = 0;
    if (cur) {
      const unsigned long long idx = p.idxList ? p.idxList[i] : p.batchFirst + i;
      u64 out[NS];
      mt_first_outputs<NS>(tea3((unsigned)idx, p.seed), out, lo, hi);
      int k = 0;
      source_sample<D>(p, [&]() { return out[k++]; }, o, d); // k is a compile-time sequence after unrolling
      if (binned)
        b = RELIEF ? bin_of_relief<D>(p, o, project_dir<D>(d)) : bin_of<D>(p, o, project_dir<D>(d));
    }
    if (havePrev) { // the previous ray of this lane: its slot has arrived
      unsigned slot = pi;
      if (binned) {
        if (RELIEF && (pbin >> 31)) { // a loose bin: its slots and its overflow region lie behind the tight bins'
          const unsigned lb = pbin & 0x7FFFFFFFu;
          if (ppos < p.binCap)
            slot = p.looseSlotBase + lb * p.binCap + ppos;
          else
            slot = p.looseSlotBase + p.looseNumBins * p.binCap + atomicAdd(&p.binCount[p.looseCntBase + p.looseNumBins], 1u);
        } else if (ppos < p.binCap)
          slot = pbin * p.binCap + ppos;
        else
          slot = p.numBins * p.binCap + atomicAdd(&p.binCount[p.numBins], 1u); // < ovCap by construction
      }
      // record = {A, B} (32 B) [+ the RNG cursors {s[k], s[k+156]} (16 B) when the particle keeps going]
      if (KEEP) {
        // compact: the origin's two free coordinates, the direction, the index and s[k+156]; the tracer knows the source
        // plane and the draw count and rebuilds s[k] from the seed (vr_types.hpp)
        float4 *rec = reinterpret_cast<float4 *>(p.slotRec) + (size_t)2 * slot;
        rec[0] = make_float4(getc(po, p.firstDir), getc(po, p.secondDir), pd.x, pd.y);
        rec[1] = make_float4(pd.z, __uint_as_float(pi), __uint_as_float((unsigned)(phi & 0xFFFFFFFFull)),
                             __uint_as_float((unsigned)(phi >> 32)));
      } else {
        float4 *rec = reinterpret_cast<float4 *>(p.slotRec) + (size_t)2 * slot;
        rec[0] = make_float4(po.x, po.y, po.z, pd.x);
        rec[1] = make_float4(pd.y, pd.z, __uint_as_float(pi), __uint_as_float((unsigned)NS));
      }
    }
    if (!cur)
      break;
    if (binned)
      ppos = atomicAdd(&p.binCount[(RELIEF && (b >> 31)) ? p.looseCntBase + (b & 0x7FFFFFFFu) : b], 1u); // (answer used in the next pass)
    po = o;
    pd = d;
    pi = i;
    pbin = b;
    phi = hi;
    havePrev = true;
  }
}

// General generator (tilted primary direction: the rejection loop makes the number
// of draws data dependent): the streaming generator from draw 0 (+ tier 2).
template <int D, bool KEEP> __global__ __launch_bounds__(VR_BLOCK) void gen_basis_kernel(const TraceParams p) {
  const unsigned tid = threadIdx.x;
  const unsigned gwave = (blockIdx.x * VR_BLOCK + tid) >> 6; // physical wave of this (bounded) grid
  u64 *scratchLane = p.rngScratch + (size_t)gwave * (312u * 64u) + (tid & 63u);
  for (unsigned i = blockIdx.x * VR_BLOCK + tid; i < p.batchCount; i += gridDim.x * VR_BLOCK) {
    const unsigned long long idx = p.idxList ? p.idxList[i] : p.batchFirst + i;
    Rng rng;
    rng_init(rng, tea3((unsigned)idx, p.seed), scratchLane);
    unsigned t2 = 0;
    V3 o, d;
    source_sample<D>(p, [&]() { return rng_next(rng, t2); }, o, d);
    gen_store<D, KEEP>(p, i, o, d, rng.k, rng.lo, rng.hi); // (k >= 156: the trace kernel rebuilds tier 2 from the seed)
  }
}

// SourceGrid (raySourceGrid.hpp:25-66): origin = grid[idx % numPoints], direction from two draws
// (cosf / sinf / powf / sqrtf in float, then Normalize)
template <int D, bool KEEP> __global__ __launch_bounds__(VR_BLOCK) void gen_grid_kernel(const TraceParams p) {
  for (unsigned i = blockIdx.x * VR_BLOCK + threadIdx.x; i < p.batchCount; i += gridDim.x * VR_BLOCK) {
    const unsigned long long idx = p.idxList ? p.idxList[i] : p.batchFirst + i;
    u64 out[2], lo, hi;
    mt_first_outputs<2>(tea3((unsigned)idx, p.seed), out, lo, hi);
    const float r1 = canon_f32(out[0]), r2 = canon_f32(out[1]);
    const float *g = p.gridPoints + 3 * (size_t)(idx % p.gridCount);
    const V3 o = mk(g[0], g[1], g[2]);
    const float tt = glibc_powf(r2, p.eeGrid);
    const float ang = (float)(3.14159265358979323846 * 2.f * (double)r1);
    float sn, cs;
    glibc_sincosf(ang, sn, cs);
    V3 d = mk(0.f, 0.f, 0.f);
    setc(d, p.rayDir, p.posNeg * sqrtf(tt));
    setc(d, p.firstDir, cs * sqrtf(1.f - tt));
    setc(d, p.secondDir, D == 2 ? 0.f : sn * sqrtf(1.f - tt));
    vnormalize(d);
    gen_store<D, KEEP>(p, i, o, d, 2u, lo, hi);
  }
}

// Rays produced by a host-side Source callback (raySource.hpp:10-19): origin, direction and the
// number of engine outputs the callback consumed; the record's RNG cursors continue from there
template <int D, bool KEEP> __global__ __launch_bounds__(VR_BLOCK) void gen_host_kernel(const TraceParams p) {
  const unsigned tid = threadIdx.x;
  const unsigned gwave = (blockIdx.x * VR_BLOCK + tid) >> 6;
  u64 *scratchLane = p.rngScratch + (size_t)gwave * (312u * 64u) + (tid & 63u);
  for (unsigned i = blockIdx.x * VR_BLOCK + tid; i < p.batchCount; i += gridDim.x * VR_BLOCK) {
    const unsigned long long idx = p.idxList ? p.idxList[i] : p.batchFirst + i;
    const V3 o = mk(p.hostOrg[3 * idx], p.hostOrg[3 * idx + 1], p.hostOrg[3 * idx + 2]);
    const V3 d = mk(p.hostDir[3 * idx], p.hostDir[3 * idx + 1], p.hostDir[3 * idx + 2]);
    Rng rng;
    rng_init(rng, tea3((unsigned)idx, p.seed), scratchLane);
    if (KEEP) {
      unsigned t2 = 0;
      const unsigned k = p.hostDraws ? p.hostDraws[idx] : 0u;
      for (unsigned j = 0; j < k && j < 156u; ++j)
        (void)rng_next(rng, t2);
      rng.k = k; // (k >= 156: the trace kernel rebuilds the full state from the seed and skips k outputs)
    }
    gen_store<D, KEEP>(p, i, o, d, rng.k, rng.lo, rng.hi);
  }
}

// No sort bins (bin_of's far-plane crossing supposes an origin on the source plane): the records stay in index order — a
// wave of 64 consecutive rays shares its origin wherever a point has 64 rays or more — as one overflow region behind
// numBins == 0 bins, which the trace kernel reads in chunks of binCap.  (Bins keyed on the origin's cell were measured
// slower in both kernels: DESIGN.md 5.1.)
template <int D, bool KEEP> __global__ __launch_bounds__(VR_BLOCK) void gen_surface_kernel(const TraceParams p) {
  if (p.binCount && blockIdx.x == 0 && threadIdx.x == 0)
    p.binCount[p.numBins] = p.batchCount;
  for (unsigned i = blockIdx.x * VR_BLOCK + threadIdx.x; i < p.batchCount; i += gridDim.x * VR_BLOCK) {
    const unsigned long long idx = p.idxList ? p.idxList[i] : p.batchFirst + i;
    V3 o, d;
    float w;
    u64 lo, hi;
    surface_sample(p, (unsigned)idx, o, d, w, lo, hi);
    gen_write<KEEP>(p, p.binCount ? p.numBins * p.binCap + i : i, i, o, d, 2u, lo, hi);
    // the start weight goes where the trace kernel reads a host ray's: hostWeights[global ray index] (4 bytes per ray
    // of the batch; indexing the per-point table there instead would put a division into every general trace kernel,
    // whose register allocation does not take it: 18 -> 48 spilled VGPRs in the 3-D disk kernel)
    if (p.hostWeights)
      const_cast<float *>(p.hostWeights)[p.batchFirst + i] = w;
  }
}
#endif // VR_USER_MODULE

} // namespace vr
