// vr_tile_buckets.hpp — the tile-bucket pipeline of a lattice-lanes launch (trace_kernel MODE_ABSORB_FLAT_LATTICE_LANES):
// a generator that files the rays by lattice TILE with one global atomic per (chunk, tile) in place of one per ray, and a
// kernel that finishes a tile's rays against the tile's disks held in LDS.  vr_lattice_tiles.hpp has the tiles'
// arithmetic, vr_trace.hip the two launchers, DESIGN.md 5.2 the sizing.
//
// gen_kernel's returning atomicAdd on binCount[b] lands on a random one of ~2 10^6 bins and every one of them reaches the
// memory side; the generator is 1.0 ms faster without it.  Rays whose end is decided by the four disks at the corners of
// their own lattice cell need no fine sort, only their disks near by: a tile of the lattice in LDS.  (That the chip's RATE
// for such atomics bounds the generator was the hypothesis this was built on; the measurements did not confirm it:
// DESIGN.md 5.1, "Bound, revisited".)
//
// A ray is SIMPLE when it is wall-free (planar_wall_free) and its point is valid (planar_round_valid without a wall): the
// lattice-lanes kernel would find its closest hit among the four corners of the point's cell, and no wall before it
// (vr_planar_disks.hpp (3)).  gen_tile_kernel sends the simple rays to their tile's bucket and every other ray — and a
// simple one whose bucket is full — to the record stream's overflow region, gen_kernel's record for it.  tile_trace_kernel
// ends the rays that hit the front of a disk: the closest-hit rule, the `near` / `sel` crediting rule and the counters of
// the lattice-lanes kernel's DIRECT form on the same record bits.  A bucket ray without such a hit (a hole in the cloud, a
// back-face hit) is copied to the overflow region untouched.  The lattice-lanes kernel then traces the overflow region as
// it always has: every ray is finished by one of the two kernels with the arithmetic of trace_kernel, and the flux sums
// and the counters are integers — the results are those of the launch without tile buckets, bit for bit.
#pragma once
#include "vr_generate.hpp"
#include "vr_lattice_tiles.hpp"
#include "vr_trace_kernel.hpp"

namespace vr {

constexpr unsigned VR_TILE_TRACE_BLOCK = 1024; // threads of a tile block: one block per CU holds the largest tile (101 KB)
constexpr unsigned VR_TILE_NO_KEY = 0xFFFFFFFFu;
static_assert(VR_TILE_MAX_TILES <= (1u << 20), "a staged key is tile << 12 | rank");

// what both kernels read of the launch's frame (p.wallTable: the walls' 96 floats, then vr_frame.hpp's words)
struct TileFrame {
  int pa, b1, b2, a1, a2;      // the plane's axis, its in-plane axes, the two wall axes
  float s, coord, radius, thr; // the normal's +-1, the centres' coordinate along pa, the radius, the neighbour test's threshold
  PlanarWallRect wr, wi;
  float sb[4];
  int n1, n2;
  float invD, phase1, phase2;
};
__device__ __forceinline__ TileFrame tile_frame(const float *wallS) {
  TileFrame f;
  f.pa = __float_as_int(wallS[VR_F_PD_AXIS]);
  planar_in_plane_axes(f.pa, f.b1, f.b2);
  f.a1 = __float_as_int(wallS[VR_F_FIRSTDIR]);
  f.a2 = __float_as_int(wallS[VR_F_SECONDDIR]);
  f.s = wallS[VR_F_UD_N + f.pa];
  f.coord = wallS[VR_F_PD_COORD];
  f.radius = wallS[VR_F_UD_RADIUS];
  f.thr = wallS[VR_F_UD_T];
  f.wr = PlanarWallRect{wallS[VR_F_LO1], wallS[VR_F_LO1 + 1], wallS[VR_F_LO1 + 2], wallS[VR_F_LO1 + 3]};
  f.wi = PlanarWallRect{wallS[VR_F_PR_IN], wallS[VR_F_PR_IN + 1], wallS[VR_F_PR_IN + 2], wallS[VR_F_PR_IN + 3]};
  for (int k = 0; k < 4; ++k)
    f.sb[k] = wallS[VR_F_PR_SB + k];
  f.n1 = __float_as_int(wallS[VR_F_PL_N1]);
  f.n2 = __float_as_int(wallS[VR_F_PL_N2]);
  f.invD = wallS[VR_F_PL_INVD];
  f.phase1 = wallS[VR_F_PL_PHASE1];
  f.phase2 = wallS[VR_F_PL_PHASE2];
  return f;
}
// the round's point of a fresh ray, with the operands trace_kernel hands planar_round_point (PLANAR_ROUND, tnear = 1e-4)
__device__ __forceinline__ PlanarRound tile_round_point(const TileFrame &f, const V3 &org, const V3 &dir) {
  return planar_round_point(true, org.x, org.y, org.z, dir.x, dir.y, dir.z, getc(org, f.pa), getc(dir, f.pa) * f.s, 1e-4f, f.coord, f.s,
                            f.radius, f.thr);
}

// ---------------------------------------------------------------------------
// gen_tile_kernel: gen_kernel<3, false, false>'s rays (the same mt_first_outputs<4> and source_sample), filed by tile.
// A block gathers a chunk of CHUNK consecutive rays: each ray takes its rank among the chunk's rays of its tile from an LDS
// counter (a returning ds_add) and is staged in LDS — five words, the origin's coordinate on the source axis is the
// launch's — then ONE global atomic per non-empty (chunk, tile) reserves the run in the tile's bucket, and the records go
// out at run + rank.  The rays that are not simple are one more "tile" of the chunk, whose bucket is the record stream's
// overflow region (cursor binCount[numBins]): a tile-bucket launch has no sort bins — the rays that cross a wall land
// within a cell or two of the walls, a uniform grid sized for their number overflows there and one sized for their
// density is as large as the whole batch's — and the lattice-lanes kernel reads the region in chunks of binCap rays as it
// reads a surface source's.  A ray whose bucket is full joins them by an atomic of its own (the sizing makes that rare).
// ---------------------------------------------------------------------------
template <unsigned BLOCK, unsigned CHUNK>
__global__ __launch_bounds__(BLOCK) void gen_tile_kernel(const TraceParams p, const TileParams tp) {
  static_assert(CHUNK <= 4096u && CHUNK % BLOCK == 0u, "a staged key is tile << 12 | rank");
  __shared__ float wallS[VR_WALL_TABLE];
  __shared__ unsigned cntS[VR_TILE_MAX_TILES + 1]; // per tile: the chunk's count, then its run's first slot; [numTiles]: the other rays
  __shared__ unsigned stageS[6 * CHUNK];           // [word][ray of the chunk]: o[firstDir], o[secondDir], d.xyz, key
  const unsigned tid = threadIdx.x;
  if (tid < VR_WALL_TABLE)
    wallS[tid] = p.wallTable[tid];
  __syncthreads();
  const TileFrame f = tile_frame(wallS);
  const unsigned numTiles = tp.numTiles < VR_TILE_MAX_TILES ? tp.numTiles : VR_TILE_MAX_TILES;
  const unsigned ovBase = p.numBins * p.binCap; // first slot of the overflow region
  unsigned toBins = 0u;
  for (unsigned long long base = (unsigned long long)blockIdx.x * CHUNK; base < p.batchCount;
       base += (unsigned long long)gridDim.x * CHUNK) {
    for (unsigned t = tid; t <= numTiles; t += BLOCK)
      cntS[t] = 0u;
    __syncthreads();
#pragma unroll 1
    for (unsigned r = tid; r < CHUNK; r += BLOCK) {
      unsigned key = VR_TILE_NO_KEY;
      const unsigned long long i64 = base + r;
      if (i64 < p.batchCount) {
        const unsigned i = (unsigned)i64;
        u64 out[4], lo, hi;
        mt_first_outputs<4>(tea3((unsigned)(p.batchFirst + i), p.seed), out, lo, hi);
        V3 o, d;
        int k = 0;
        source_sample<3>(p, [&]() { return out[k++]; }, o, d);
        const V3 dir = project_dir<3>(d);
        const PlanarRound rp = tile_round_point(f, o, dir);
        const V3 q = mk(rp.qx, rp.qy, rp.qz);
        const float u = getc(q, f.b1), v = getc(q, f.b2);
        const bool simple = planar_wall_free(getc(o, f.a1), getc(o, f.a2), getc(q, f.a1), getc(q, f.a2), f.wr, f.wi) &&
                            planar_round_valid(rp, u, v, 3.402823466e+38f, f.sb[0], f.sb[1], f.sb[2], f.sb[3]);
        const int t1 = lattice_tile_of(lattice_lane_corner(u, f.phase1, f.invD, f.n1), tp.shift);
        const int t2 = lattice_tile_of(lattice_lane_corner(v, f.phase2, f.invD, f.n2), tp.shift);
        unsigned tile = (unsigned)t2 * (unsigned)tp.tiles1 + (unsigned)t1;
        if (!(simple && t1 >= 0 && t1 < tp.tiles1 && t2 >= 0 && t2 < tp.tiles2 && tile < numTiles))
          tile = numTiles;
        key = (tile << 12) | atomicAdd(&cntS[tile], 1u); // (the rank: below CHUNK)
        stageS[0 * CHUNK + r] = __float_as_uint(getc(o, p.firstDir));
        stageS[1 * CHUNK + r] = __float_as_uint(getc(o, p.secondDir));
        stageS[2 * CHUNK + r] = __float_as_uint(d.x);
        stageS[3 * CHUNK + r] = __float_as_uint(d.y);
        stageS[4 * CHUNK + r] = __float_as_uint(d.z);
      }
      stageS[5 * CHUNK + r] = key;
    }
    __syncthreads();
    for (unsigned t = tid; t <= numTiles; t += BLOCK) {
      const unsigned n = cntS[t];
      cntS[t] = n ? atomicAdd(t < numTiles ? &tp.tileCount[t] : &p.binCount[p.numBins], n) : 0u;
    }
    __syncthreads();
#pragma unroll 1
    for (unsigned r = tid; r < CHUNK; r += BLOCK) {
      const unsigned key = stageS[5 * CHUNK + r];
      if (key == VR_TILE_NO_KEY)
        continue;
      const unsigned tile = key >> 12, i = (unsigned)(base + r);
      const unsigned long long pos = (unsigned long long)cntS[tile] + (key & 0xFFFu);
      V3 o = mk(0.f, 0.f, 0.f), d;
      setc(o, p.rayDir, p.srcCoord);
      setc(o, p.firstDir, __uint_as_float(stageS[0 * CHUNK + r]));
      setc(o, p.secondDir, __uint_as_float(stageS[1 * CHUNK + r]));
      d = mk(__uint_as_float(stageS[2 * CHUNK + r]), __uint_as_float(stageS[3 * CHUNK + r]), __uint_as_float(stageS[4 * CHUNK + r]));
      unsigned long long slot;
      if (tile < numTiles && pos < tp.tileCap) {
        slot = (unsigned long long)tp.slotBase + (unsigned long long)tile * tp.tileCap + pos;
      } else {
        // not simple: the chunk's run in the overflow region; a full bucket: one more slot of it
        slot = (unsigned long long)ovBase + (tile < numTiles ? (unsigned long long)atomicAdd(&p.binCount[p.numBins], 1u) : pos);
        ++toBins;
        if (slot >= (unsigned long long)ovBase + p.ovCap) // (cannot be: the region holds a whole batch)
          continue;
      }
      gen_write<false>(p, (unsigned)slot, i, o, d, 4u, 0ull, 0ull);
    }
    __syncthreads(); // (the next chunk clears the counters)
  }
  const unsigned long long s = wave_sum(toBins);
  if ((tid & 63u) == 0u && s)
    atomicAdd(&p.counters[C_TILE_FALLBACK], s);
}

// ---------------------------------------------------------------------------
// tile_trace_kernel: block b takes slice b % slices of bucket b / slices.  It files the tile's (T + 1)^2 lattice points —
// {leaf position, centre}, original id, a zeroed counter; VR_LATTICE_EMPTY for a hole and for a point outside the table —
// in LDS, streams its slice of the bucket, and per ray: the round's point from the record, the four corners of its cell
// from LDS through planar_round_cand and hit_update_lds, and for a front-side hit the `near` / `sel` rule of trace_kernel's
// lattice-lanes crediting with a ds_add per selected disk.  Then the non-zero counters go out as count << 40.
// Every LDS index is a lattice_tile_slot (below (T + 1)^2) or 0, every table index lies inside the table or is 0.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(VR_TILE_TRACE_BLOCK) void tile_trace_kernel(const TraceParams p, const TileParams tp) {
  extern __shared__ uint4 tileDyn[];
  __shared__ float wallS[VR_WALL_TABLE];
  const unsigned tid = threadIdx.x, lane = tid & 63u;
  const unsigned tile = blockIdx.x / tp.slices, slice = blockIdx.x % tp.slices;
  if (tile >= tp.numTiles)
    return;
  const unsigned filled = tp.tileCount[tile] < tp.tileCap ? tp.tileCount[tile] : tp.tileCap;
  const unsigned first = (unsigned)((unsigned long long)filled * slice / tp.slices);
  const unsigned last = (unsigned)((unsigned long long)filled * (slice + 1u) / tp.slices);
  if (first >= last) // (the whole block: nothing before this point synchronises)
    return;
  if (tid < VR_WALL_TABLE)
    wallS[tid] = p.wallTable[tid];
  __syncthreads();
  const TileFrame f = tile_frame(wallS);
  const int shift = tp.shift < VR_TILE_SHIFT_MIN ? VR_TILE_SHIFT_MIN : (tp.shift > VR_TILE_SHIFT_MAX ? VR_TILE_SHIFT_MAX : tp.shift);
  const int W = lattice_tile_width(shift);
  const unsigned P = (unsigned)(W * W);
  U4 *const rec = reinterpret_cast<U4 *>(tileDyn);
  unsigned *const ids = reinterpret_cast<unsigned *>(rec + P);
  unsigned *const cnt = ids + P;
  const int ti = (int)(tile % (unsigned)tp.tiles1), tj = (int)(tile / (unsigned)tp.tiles1);
  typedef const __attribute__((address_space(1))) unsigned *GlobalU32;
  const GlobalU32 table = reinterpret_cast<GlobalU32>(frame_addr(wallS, VR_F_PL_PTR_LO));
  const float4 *__restrict__ prims = reinterpret_cast<const float4 *>(p.prims);
  {
    const int i0 = lattice_tile_first(ti, shift), j0 = lattice_tile_first(tj, shift);
    for (unsigned k = tid; k < P; k += VR_TILE_TRACE_BLOCK) {
      const int lj = (int)k / W, li = (int)k - lj * W;
      const int i = i0 + li, j = j0 + lj;
      const bool inT = (i >= 0) & (i < f.n1) & (j >= 0) & (j < f.n2);
      unsigned pos = table[inT ? (unsigned)j * (unsigned)f.n1 + (unsigned)i : 0u];
      pos = inT ? pos : VR_LATTICE_EMPTY;
      const bool present = pos != VR_LATTICE_EMPTY;
      const size_t rp = present ? (size_t)pos : (size_t)0;
      const float4 r0 = prims[2 * rp];
      const unsigned orig = __float_as_uint(prims[2 * rp + 1].w);
      rec[k] = mk_u4(pos, __float_as_uint(r0.x), __float_as_uint(r0.y), __float_as_uint(r0.z));
      ids[k] = orig;
      cnt[k] = 0u;
    }
  }
  __syncthreads();
  const float4 *__restrict__ rayAB = reinterpret_cast<const float4 *>(p.slotRec) + 2 * ((size_t)tp.slotBase + (size_t)tile * tp.tileCap);
  float4 *const ovRec = reinterpret_cast<float4 *>(p.slotRec) + 2 * (size_t)p.numBins * p.binCap;
  const V3 normal = mk(wallS[VR_F_UD_N], wallS[VR_F_UD_N + 1], wallS[VR_F_UD_N + 2]);
  const float dist = p.nbDist, dist2 = dist * dist;
  unsigned done = 0u, handedOn = 0u;
  // (whole waves go round together: the hand-over below votes)
  for (unsigned sBase = first + (tid & ~63u); sBase < last; sBase += VR_TILE_TRACE_BLOCK) {
    const unsigned s = sBase + lane;
    const bool on = s < last;
    const float4 a = rayAB[2 * (size_t)(on ? s : first)], b = rayAB[2 * (size_t)(on ? s : first) + 1];
    const V3 org = mk(a.x, a.y, a.z), rayDirection = mk(a.w, b.x, b.y);
    const V3 dir = project_dir<3>(rayDirection);
    const PlanarRound rp = tile_round_point(f, org, dir);
    const V3 q = mk(rp.qx, rp.qy, rp.qz);
    const float u = getc(q, f.b1), v = getc(q, f.b2);
    const int ci = lattice_lane_corner(u, f.phase1, f.invD, f.n1), cj = lattice_lane_corner(v, f.phase2, f.invD, f.n2);
    // (the generator's tile, from the same bits; a ray of another tile would be handed on, not tested against this one)
    const bool mineTile = lattice_tile_of(ci, shift) == ti && lattice_tile_of(cj, shift) == tj;
    HitRec h;
    hit_clear(h);
    unsigned sl[4], local = 0u, there = 0u, mine = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int slot = lattice_tile_slot(ci + (k & 1), cj + (k >> 1), ti, tj, shift);
      sl[k] = slot < 0 ? 0u : (unsigned)slot;
      const U4 cr = rec[sl[k]];
      const unsigned orig = ids[sl[k]];
      const bool present = (slot >= 0) & (cr.x != VR_LATTICE_EMPTY);
      bool ok, okLocal;
      planar_round_cand(rp, __uint_as_float(cr.y), __uint_as_float(cr.z), __uint_as_float(cr.w), ok, okLocal);
      const bool took = hit_update_lds(h, ok & present, rp.t, orig, cr.x);
      mine = took ? (unsigned)k : mine;
      local |= (unsigned)(okLocal & present) << k;
      there |= (unsigned)present << k;
    }
    // the state machine of a fresh ray's first segment: a front-side disk hit ends an absorbed ray
    const bool backface = vdot(rayDirection, normal) > 0.f;
    const bool credit = on & mineTile & (h.geom == 1) & !backface;
    if (credit) {
      ++done;
      const U4 own = rec[sl[mine]];
      const float px = __uint_as_float(own.y), py = __uint_as_float(own.z), pz = __uint_as_float(own.w);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const U4 cr = rec[sl[k]];
        const float dx = px - __uint_as_float(cr.y), dy = py - __uint_as_float(cr.z), dz = pz - __uint_as_float(cr.w);
        const float ax = fabsf(dx), ay = fabsf(dy), az = fabsf(dz);
        const bool near = (ax <= dist) & (ay <= dist) & ((p.geoD == 2) | (az <= dist)) & (((dx * dx + dy * dy) + dz * dz) <= dist2);
        const bool sel = (((there >> k) & 1u) != 0u) & ((h.pos == cr.x) | (near & (((local >> k) & 1u) != 0u)));
        if (sel)
          atomicAdd(&cnt[sl[k]], 1u);
      }
    }
    // every other ray of the bucket: its record, as it is, to the overflow region (one atomic per wave)
    const bool hand = on & !credit;
    handedOn += hand ? 1u : 0u;
    const unsigned long long hm = ballot64(hand);
    if (hm) {
      unsigned at = 0u;
      if (lane == (unsigned)(__ffsll((long long)hm) - 1))
        at = atomicAdd(&p.binCount[p.numBins], (unsigned)__popcll(hm));
      at = (unsigned)__shfl((int)at, __ffsll((long long)hm) - 1, 64);
      const unsigned pos = at + (unsigned)__popcll(hm & ((1ull << lane) - 1ull));
      if (hand && pos < p.ovCap) {
        ovRec[2 * (size_t)pos] = a;
        ovRec[2 * (size_t)pos + 1] = b;
      }
    }
  }
  // a finished ray: one trace segment, one geometry hit (trace_kernel's K_TRACES, K_GEO)
  const unsigned long long nd = wave_sum(done);
  if (lane == 0u && nd) {
    atomicAdd(&p.counters[C_TRACES], nd);
    atomicAdd(&p.counters[C_GEO], nd);
  }
  const unsigned long long nh = wave_sum(handedOn);
  if (lane == 0u && nh)
    atomicAdd(&p.counters[C_TILE_HANDED], nh);
  __syncthreads();
  unsigned long long *const fluxGlobal = p.fluxAcc + (size_t)(blockIdx.x & p.accMask) * p.accStride;
  for (unsigned k = tid; k < P; k += VR_TILE_TRACE_BLOCK) {
    const unsigned n = cnt[k];
    if (n)
      atomicAdd(&fluxGlobal[rec[k].x], (unsigned long long)n * 1099511627776ull); // unit weights: count x 2^40
  }
}

} // namespace vr
