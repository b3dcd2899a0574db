// gather_energy.cpp — the arithmetic of the energy gather (vr_gather_energy*) on the host: vr_gather.hpp alone, the text the
// kernel compiles.  tests/test_gather_energy_host.py builds it plain and with ASan + UBSan and runs it stand-alone.
//   (no argument)  the soundness of the cut for every table size M in 2 .. 256 and every count Z0 of leading zeros, 10^4
//                  random retention sequences each; and the identity "P is the angular call's T multiply for multiply".
//   draws          10^4 lines "seed prim sample u-bits E0-bits" for numpy to recompute.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "vr_gather.hpp"

using namespace vr;

static thread_local uint64_t rngState = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  rngState ^= rngState << 13;
  rngState ^= rngState >> 7;
  rngState ^= rngState << 17;
  return rngState;
}
static float uniform() { return (float)(rnd() >> 40) * 5.9604644775390625e-08f; } // [0, 1)
static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}
static float from_bits(uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
// f moved by `ulps` representable values (f > 0 and far from the ends of the range)
static float nudge(float f, int ulps) { return from_bits((uint32_t)((int32_t)bits(f) + ulps)); }

// (per thread: cut_soundness shares the table sizes out; main adds the counts up)
static thread_local unsigned long long checks = 0, failed = 0;
static void check(bool ok, const char *what, unsigned M, unsigned Z0) {
  ++checks;
  if (!ok && failed++ < 20)
    std::printf("FAILED %s (M %u Z0 %u)\n", what, M, Z0);
}

// the quantile table the draws are read through (the test has the same values)
static void quantiles(std::vector<float> &Q) {
  Q.resize(37);
  for (size_t k = 0; k < Q.size(); ++k)
    Q[k] = 10.f + 2.5f * (float)k + 0.125f * (float)(k * k);
}

static int draws() {
  std::vector<float> Q;
  quantiles(Q);
  for (int i = 0; i < 10000; ++i) {
    const uint32_t seed = (uint32_t)rnd(), prim = i % 7 == 0 ? (uint32_t)rnd() : (uint32_t)(rnd() % 100000u),
                   sample = (uint32_t)(rnd() % (1u << 22));
    const float u = gather_energy_u(gather_path_key(seed, prim, sample));
    const float E0 = gather_energy_source(Q.data(), (uint32_t)Q.size(), u, 0.f);
    std::printf("%u %u %u %u %u\n", seed, prim, sample, bits(u), bits(E0));
  }
  return 0;
}

// a retention as a path can meet it: exactly 1, exactly 0, a hair below 1, or anything between (one draw: the low bits
// choose, the high 24 are the value)
static float retention() {
  const uint64_t v = rnd();
  const unsigned kind = (unsigned)(v & 7u);
  const float f = (float)(v >> 40) * 5.9604644775390625e-08f;
  if (kind == 0)
    return 1.f;
  if (kind == 1)
    return 0.f;
  if (kind == 2)
    return nudge(1.f, -(int)(1 + ((v >> 3) & 3u) % 3u));
  if (kind == 3)
    return 0.5f + 0.5f * f;
  return f;
}

// table sizes first, first + stride, ...
static void cut_soundness(uint32_t first, uint32_t stride) {
  constexpr int SEQUENCES = 10000, STEPS = 4;
  std::vector<float> Y(GATHER_LAW_MAX);
  for (uint32_t M = GATHER_LAW_MIN + first; M <= GATHER_LAW_MAX; M += stride) {
    for (uint32_t Z0 = 0; Z0 <= M; ++Z0) {
      for (uint32_t k = 0; k < M; ++k)
        Y[k] = k < Z0 ? 0.f : 0.25f + uniform();
      check(gather_energy_zeros(Y.data(), M) == Z0, "the leading zeros are counted", M, Z0);
      if (Z0 < 2u)
        continue; // (the rule is off: the entry points pass zeros = 0)
      const float boundary = (float)(Z0 - 1u) / (float)(M - 1u);
      for (int q = 0; q < SEQUENCES; ++q) {
        // the energy at the source: within a few representable values of the boundary, or anywhere up to 1.25
        float E0, energyMax;
        const uint64_t v = rnd();
        const unsigned kind = (unsigned)(v & 3u);
        const int ulps = (int)((v >> 2) % 9u) - 4;
        if (kind < 2u) {
          E0 = nudge(boundary, ulps);
          energyMax = 1.f;
        } else if (kind == 2u) {
          energyMax = 0.5f + 100.f * ((float)(v >> 40) * 5.9604644775390625e-08f);
          E0 = nudge(boundary, ulps) * energyMax;
        } else {
          energyMax = 0.5f + 100.f * uniform();
          E0 = 1.25f * uniform() * energyMax;
        }
        float P = 1.f, e = gather_energy_arrival(E0, P, energyMax);
        bool fired = gather_energy_cut(e, M, Z0);
        if (fired)
          check(gather_law(Y.data(), M, e) == 0.f, "a sample cut before its walk reads 0", M, Z0);
        for (int s = 0; s < STEPS; ++s) {
          const float r = retention(), eps[2] = {r, r};
          P = gather_energy_retain(P, eps, 2u, 0.375f); // (a constant table: any mu reads r)
          const float eNew = gather_energy_arrival(E0, P, energyMax);
          check(eNew <= e, "e never rises", M, Z0);
          e = eNew;
          const bool now = gather_energy_cut(e, M, Z0);
          check(now || !fired, "the rule keeps holding once it has fired", M, Z0);
          fired = fired || now;
          if (fired)
            check(gather_law(Y.data(), M, e) == 0.f, "after the rule has fired the yield reads exactly 0", M, Z0);
        }
      }
    }
  }
}

// sticking 0, sourceEnergy = energyMax = 1, energyYield {0, 1}, retentionLaw R: P is the angular call's T under the
// reflectivity law R, multiply for multiply, and the weight has that call's bits
static void identity() {
  const float Y01[2] = {0.f, 1.f};
  std::vector<float> R(GATHER_LAW_MAX);
  for (int q = 0; q < 10000; ++q) {
    const uint32_t MR = GATHER_LAW_MIN + (uint32_t)(rnd() % (GATHER_LAW_MAX - GATHER_LAW_MIN + 1u));
    for (uint32_t k = 0; k < MR; ++k)
      R[k] = rnd() % 16u == 0 ? (rnd() % 2u ? 1.f : 0.f) : uniform();
    const float g = 1.f + uniform(), n = 1.f + 3.f * uniform(), cEnd = uniform();
    float T = 1.f, P = 1.f;
    bool absorbed = false;
    const int steps = (int)(rnd() % 9u);
    for (int s = 0; s < steps && !absorbed; ++s) {
      const float mu = uniform();
      T = gather_path_throughput(T, 1.f); // rho = 1 - sticking
      T = gather_path_throughput_law(T, R.data(), MR, mu);
      P = gather_energy_retain(P, R.data(), MR, mu);
      check(bits(T) == bits(P), "P is T multiply for multiply", MR, 1u);
      absorbed = T == 0.f; // (the angular path ends there, weight 0; the energy path weighs 0 through e = 0)
    }
    const float wAngular = absorbed ? 0.f : gather_path_weight_laws(GATHER_END_MISS, g, n, cEnd, T, nullptr, 0u, 1.f, nullptr, 0u, 0.f);
    const float e = gather_energy_arrival(1.f, P, 1.f);
    check(bits(e) == bits(P), "e is P where sourceEnergy = energyMax = 1", MR, 1u);
    const float base = gather_path_weight_laws(GATHER_END_MISS, g, n, cEnd, 1.f, nullptr, 0u, 1.f, nullptr, 0u, 0.f);
    const float wEnergy = gather_energy_weight(base, Y01, 2u, e);
    check(gather_q(wEnergy, 1024.f) == gather_q(wAngular, 1024.f) && (absorbed || bits(wEnergy) == bits(wAngular)),
          "the weight has the angular call's bits", MR, 1u);
    // an all-ones yield of any M leaves the angular weight alone
    const uint32_t M1 = GATHER_LAW_MIN + (uint32_t)(rnd() % (GATHER_LAW_MAX - GATHER_LAW_MIN + 1u));
    std::vector<float> ones(M1, 1.f);
    check(bits(gather_energy_weight(wAngular, ones.data(), M1, 1.25f * uniform())) == bits(wAngular), "an all-ones yield changes no bit",
          M1, 0u);
  }
}

int main(int argc, char **argv) {
  if (argc > 1 && !std::strcmp(argv[1], "draws"))
    return draws();
  // the table sizes are shared out over a few threads, each with its own generator and counts
  unsigned T = std::thread::hardware_concurrency();
  T = T < 1u ? 1u : (T > 8u ? 8u : T);
  std::vector<unsigned long long> done(T, 0), bad(T, 0);
  std::vector<std::thread> pool;
  for (unsigned t = 0; t < T; ++t)
    pool.emplace_back([t, T, &done, &bad] {
      rngState += 0x632BE59BD9B4E019ull * (t + 1u);
      cut_soundness(t, T);
      done[t] = checks, bad[t] = failed;
    });
  for (auto &th : pool)
    th.join();
  identity();
  for (unsigned t = 0; t < T; ++t)
    checks += done[t], failed += bad[t];
  std::printf("%llu checks\n%llu failed checks\n", checks, failed);
  return failed ? 1 : 0;
}
