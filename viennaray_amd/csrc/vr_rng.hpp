// vr_rng.hpp — the per-ray mt19937_64 stream, the canonical floats and the power-cosine sample (gfx950).
#pragma once
#include "vr_libm.hpp"
#include "vr_math.hpp"
namespace vr {

// ---------------------------------------------------------------------------
// Per-ray RNG: mt19937_64 seeded with tea<3>(idx, seed)
// (reference: rayTraceKernel.hpp:100,120-121; engine = std::mt19937_64).
//
// A fresh 312-word engine per ray is what makes the reference's CPU loop
// expensive; on the GPU the stream is evaluated lazily from its recurrence
//   s[0] = seed, s[j] = 6364136223846793005 (s[j-1] ^ s[j-1]>>62) + j  (j < 312)
//   s[n+312] = s[n+156] ^ tw(s[n], s[n+1]),  output k = temper(s[k+312])
// Tier 1: outputs 0..155 depend on seeding words only (s[k], s[k+1], s[k+156]); the
//   generator reaches s[156] once per ray (the unavoidable 156 sequential steps) and
//   from there every draw advances two cursors by one step each (struct Rng below).
// Tier 2: a ray that draws more than 156 numbers builds the whole 312-word state in a
//   per-lane global scratch slab ([word][lane] so a wave's accesses coalesce) and
//   continues with the textbook block twist.
// ---------------------------------------------------------------------------

__device__ __forceinline__ unsigned tea3(unsigned v0, unsigned v1) {
  unsigned s0 = 0;
#pragma unroll
  for (int n = 0; n < 3; ++n) {
    s0 += 0x9e3779b9u;
    v0 += ((v1 << 4) + 0xa341316cu) ^ (v1 + s0) ^ ((v1 >> 5) + 0xc8013ea4u);
    v1 += ((v0 << 4) + 0xad90777du) ^ (v0 + s0) ^ ((v0 >> 5) + 0x7e95761eu);
  }
  return v0;
}

__device__ __forceinline__ u64 mt_step(u64 p, unsigned j) { return 6364136223846793005ull * (p ^ (p >> 62)) + j; }
// The same step for the generator's seeding chain (step index a literal after unrolling), written over 32-bit
// halves with the multiplier's halves held in VGPRs: v_mad_u64_u32 can then take the step index as its scalar
// 64-bit addend (gfx9 VOP3: one scalar source per instruction) — 6 VALU per step (3 of them multiplies)
// instead of the 7 + a 64-bit add the compiler makes of the one-line form.
// (The high word by two more v_mad_u64_u32 chained onto the first — 5 VALU + a register move — issues in 20.1
//  SIMD-cycles per step against 24.4 in isolation (tools/mt_step_variants.py, vr_bench.hip kind 6), but the chip
//  then holds 2.0 - 2.27 GHz instead of 2.39, and the generator, which already runs at 1.9 GHz, got SLOWER: 4.66 ->
//  4.8 - 4.95 ms.  The generator is bound by power, not by issue slots; v_mul_lo_u32 is the cheaper multiply.)
struct MtMul {
  unsigned al, ah;
};
__device__ __forceinline__ MtMul mt_mul_init() {
  MtMul m{0x4C957F2Du, 0x5851F42Du}; // 6364136223846793005 = 0x5851F42D4C957F2D
  asm volatile("" : "+v"(m.al), "+v"(m.ah));
  return m;
}
__device__ __forceinline__ u64 mt_step_v(const MtMul &m, u64 p, unsigned j) {
  const unsigned xh = (unsigned)(p >> 32);
  const unsigned t = (unsigned)p ^ (xh >> 30); // low word of p ^ (p >> 62); the high word is unchanged
  u64 r; // = t * al + j, the index in a scalar register pair (written out: LLVM's constant hoisting otherwise
         //   rebuilds the indices from a base held in VGPRs, at two more VALU per step)
  asm("v_mad_u64_u32 %0, vcc, %1, %2, %3" : "=v"(r) : "v"(t), "v"(m.al), "s"((u64)j) : "vcc");
  const unsigned hi = (unsigned)(r >> 32) + t * m.ah + xh * m.al;
  return ((u64)hi << 32) | (unsigned)r;
}
__device__ __forceinline__ u64 mt_twist(u64 a, u64 b, u64 c) {
  u64 y = (a & 0xFFFFFFFF80000000ull) | (b & 0x7FFFFFFFull);
  return c ^ (y >> 1) ^ ((b & 1ull) ? 0xB5026F5AA96619E9ull : 0ull);
}
__device__ __forceinline__ u64 mt_temper(u64 v) {
  v ^= (v >> 29) & 0x5555555555555555ull;
  v ^= (v << 17) & 0x71D67FFFEDA60000ull;
  v ^= (v << 37) & 0xFFF7EEE000000000ull;
  v ^= (v >> 43);
  return v;
}

// Streaming form of the first 156 outputs: output k = temper(s[k+156] ^ tw(s[k], s[k+1]))
// depends on three words of the SEEDING recurrence only, and both cursors advance by one
// mt_step per draw.  A ray therefore carries {k, lo = s[k], hi = s[k+156]} (16 B + a
// counter) and every draw costs two 64-bit multiply-adds — no tape, no LDS, no state
// array — until draw 156, where the full 312-word state is needed (tier 2).
struct Rng {
  unsigned seed;   // engine seed (32 bit)
  unsigned k;      // index of the next output
  unsigned pos;    // tier 2: position in the 312-word block, 0xFFFFFFFF = not built
  u64 lo, hi;      // s[k], s[k+156] while k < 156
  u64 *scratch;    // global, this lane's column: scratch[word * 64]
};

__device__ __forceinline__ void rng_resume(Rng &r, unsigned seed, unsigned k, u64 lo, u64 hi) {
  r.seed = seed;
  r.k = k;
  r.pos = 0xFFFFFFFFu;
  r.lo = lo;
  r.hi = hi;
}

// cold start: 156 steps of the recurrence to reach s[156]
__device__ __forceinline__ void rng_init(Rng &r, unsigned seed, u64 *scratchLane) {
  const MtMul m = mt_mul_init();
  u64 x = seed;
#pragma unroll 39
  for (int j = 1; j <= 156; ++j)
    x = mt_step_v(m, x, j);
  rng_resume(r, seed, 0, (u64)seed, x);
  r.scratch = scratchLane;
}

// First K outputs of the engine, all in registers (static indexing): what the
// generator needs when the number of draws is known at compile time.  Also returns the
// streaming cursors {s[K], s[K+156]} for the draws that follow.
template <int K> __device__ __forceinline__ void mt_first_outputs(unsigned seed, u64 (&out)[K], u64 &lo, u64 &hi) {
  const MtMul m = mt_mul_init();
  u64 w[K + 1];
  u64 x = seed;
  w[0] = x;
#pragma unroll
  for (int j = 1; j <= K; ++j) {
    x = mt_step_v(m, x, j);
    w[j] = x;
  }
#pragma unroll 38 // (152 steps = 4 x 38: the step needs its index as a literal; deeper unrolling loses in the I-cache)
  for (int j = K + 1; j < 156; ++j)
    x = mt_step_v(m, x, j);
#pragma unroll
  for (int i = 0; i < K; ++i) {
    x = mt_step_v(m, x, 156 + i);
    out[i] = mt_temper(mt_twist(w[i], w[i + 1], x));
  }
  lo = w[K];
  hi = mt_step_v(m, x, 156 + K);
}

// (The two out-of-line tier-2 routines take the slab and the seed BY VALUE: handed a reference to the engine, the
//  whole struct had to live in scratch memory — every draw of the streaming tier stored its counter there and the
//  reflection loop waited on the vector-memory counter once per iteration.)
typedef __attribute__((address_space(1))) u64 GlobalU64; // (the tier-2 state is global memory: not through flat instructions)
__device__ __noinline__ void rng_tier2_build(GlobalU64 *s, unsigned seed) {
  u64 x = seed;
  s[0] = x;
  for (int j = 1; j < 312; ++j) {
    x = mt_step(x, j);
    s[j * 64] = x;
  }
}

__device__ __noinline__ void rng_tier2_twist(GlobalU64 *s) {
  u64 cur = s[0];
  for (int i = 0; i < 156; ++i) {
    u64 nxt = s[(i + 1) * 64];
    s[i * 64] = mt_twist(cur, nxt, s[(i + 156) * 64]);
    cur = nxt;
  }
  for (int i = 156; i < 311; ++i) {
    u64 nxt = s[(i + 1) * 64];
    s[i * 64] = mt_twist(cur, nxt, s[(i - 156) * 64]);
    cur = nxt;
  }
  s[311 * 64] = mt_twist(cur, s[0], s[155 * 64]);
}

__device__ __forceinline__ u64 rng_next(Rng &r, unsigned &tier2Count) {
  if (r.k < 156u) { // (tier 2 is only ever built at k >= 156)
    const u64 lo1 = mt_step(r.lo, r.k + 1u);
    const u64 v = mt_temper(mt_twist(r.lo, lo1, r.hi));
    r.lo = lo1;
    r.hi = mt_step(r.hi, r.k + 157u); // (meaningless after k = 155; never read again)
    ++r.k;
    return v;
  }
  if (r.pos == 0xFFFFFFFFu) {
    rng_tier2_build((GlobalU64 *)r.scratch, r.seed);
    rng_tier2_twist((GlobalU64 *)r.scratch);
    unsigned skip = r.k; // outputs already consumed by the streaming tier
    while (skip >= 312u) {
      rng_tier2_twist((GlobalU64 *)r.scratch);
      skip -= 312u;
    }
    r.pos = skip;
    ++tier2Count;
  }
  if (r.pos >= 312u) {
    rng_tier2_twist((GlobalU64 *)r.scratch);
    r.pos = 0;
  }
  u64 v = mt_temper(((GlobalU64 *)r.scratch)[r.pos * 64]);
  ++r.pos;
  ++r.k;
  return v;
}

// libstdc++ std::uniform_real_distribution<float> on a 64-bit engine:
// generate_canonical = float(u64) / 2^64, clamped below 1 (bits/random.tcc)
__device__ __forceinline__ float canon_f32(u64 v) {
  float f = (float)v * 5.42101086242752217e-20f; // 2^-64, exact scaling
  return f >= 1.0f ? 0.99999994f : f;
}
__device__ __forceinline__ double canon_f64(u64 v) {
  double f = (double)v * 5.42101086242752217e-20; // 2^-64
  return f >= 1.0 ? 0.99999999999999989 : f;
}

// raySourceRandom.hpp:70-116: one power-cosine sample in the local frame, with glibc's
// float sincosf / powf reproduced bit for bit (vr_libm.hpp), so the device traces the
// very rays the reference's CPU loop traces.
__device__ __forceinline__ void cosine_sample(float r1, float r2, float ee, float &cosTheta, float &sinTheta,
                                              float &cosPhi, float &sinPhi) {
  const float ang = (float)(3.14159265358979323846 * 2. * (double)r1); // rayUtil.hpp:247-256
  glibc_sincosf(ang, sinPhi, cosPhi);
  cosTheta = glibc_powf(r2, ee);                                      // std::pow(float, float)
  sinTheta = (float)sqrt(1. - (double)(cosTheta * cosTheta));
}

} // namespace vr
