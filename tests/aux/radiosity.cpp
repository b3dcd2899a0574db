// The arithmetic of solveRadiosity (viennaray_amd/csrc/vr_radiosity.hpp) on the host: the header the kernels include, taken
// by the host compiler with vr_gather.hpp and nothing else of the library.  tests/test_radiosity_host.py builds it plain
// and with -fsanitize=address,undefined and runs it stand-alone.
//   1. two mutually facing primitives by hand: K = 4, every link at the other primitive, rho = 1/2, direct 1
//   2. the residual over bit patterns is the float maximum for non-negative floats
//   3. the table's index at N = 2^20 + 3, K = 4100: in range, injective on a sampled set
//   4. an emission above wmax is cut, as in gather_q
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "vr_gather.hpp"
#include "vr_radiosity.hpp"

using namespace vr;

static long checks = 0, failed = 0;
#define CHECK(cond)                                                                                                    \
  do {                                                                                                                 \
    ++checks;                                                                                                          \
    if (!(cond)) {                                                                                                     \
      ++failed;                                                                                                        \
      if (failed <= 20)                                                                                                \
        std::printf("FAILED line %d: %s\n", __LINE__, #cond);                                                          \
    }                                                                                                                  \
  } while (0)

static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

// ---- 1 ----
struct Pair {
  std::vector<int32_t> links;
  int64_t direct[2];
  float rho[2] = {0.5f, 0.5f};
  Pair() : links(radiosity_link_count(2, 4), 12345) { // (entries no lane owns hold rubbish: never read)
    const uint64_t slots = radiosity_slots(2);
    for (uint32_t k = 0; k < 4; ++k) {
      links[radiosity_link_index(slots, 0, k)] = 1;
      links[radiosity_link_index(slots, 1, k)] = 0;
    }
    // direct 1: every one of the K = 4 samples... brings q(1) here (by hand: a row's direct sum is K q(1))
    direct[0] = direct[1] = 4 * gather_q(1.f, gather_wmax(4));
  }
  uint32_t solve(float tol, uint32_t maxIt, float *F, float *res) const {
    float e0[2], e1[2];
    return radiosity_solve_host(links.data(), direct, 2, 4, rho, tol, maxIt, F, e0, e1, res);
  }
};

static void two_facing_primitives() {
  const Pair p;
  float F[2], res;
  CHECK(p.solve(1e-4f, 0, F, &res) == 0 && F[0] == 1.f && F[1] == 1.f && res == 0.f); // maxIterations = 0: F_0
  // F_t = 1 + F_{t-1} / 2 exactly in this arithmetic (powers of two): 1, 1.5, 1.75, ... = 2 - 2^-t, r_t = 2^-t
  float prev = 1.f;
  for (uint32_t t = 1; t <= 20; ++t) {
    const uint32_t got = p.solve(0.f, t, F, &res);
    CHECK(got == t);
    CHECK(F[0] == F[1] && F[0] == 2.f - std::ldexp(1.f, -(int)t));
    CHECK(F[0] > prev && F[0] < 2.f); // monotone, below the fixed point
    CHECK(res == std::ldexp(1.f, -(int)t));
    prev = F[0];
  }
  // the stopping rule: the first t with 2^-t <= tolerance
  for (int k = 1; k <= 12; ++k) {
    const float tol = std::ldexp(1.f, -k);
    CHECK(p.solve(tol, 1000, F, &res) == (uint32_t)k && res == tol && std::fabs(F[0] - 2.f) <= tol);
    CHECK(p.solve(tol * 1.5f, 1000, F, &res) == (uint32_t)k);
    CHECK(p.solve(tol * 0.75f, 1000, F, &res) == (uint32_t)k + 1u);
  }
  const uint32_t t = p.solve(1e-4f, 1000, F, &res);
  CHECK(t == 14 && res <= 1e-4f && std::fabs(F[0] - 2.f) <= 1e-4f && std::fabs(F[1] - 2.f) <= 1e-4f);
  // tolerance 0 runs until nothing changes bit for bit (the int64 sum reaches 2 q(1) and stays), within maxIterations
  const uint32_t t0 = p.solve(0.f, 1000, F, &res);
  CHECK(t0 < 1000 && res == 0.f && F[0] == 2.f);
  CHECK(p.solve(0.f, 7, F, &res) == 7 && res == std::ldexp(1.f, -7));
  // a row without links stays at its direct flux; rho = 0 stops everything after one iteration
  Pair q;
  q.rho[0] = q.rho[1] = 0.f;
  CHECK(q.solve(1e-4f, 1000, F, &res) == 1 && F[0] == 1.f && res == 0.f);
  Pair r;
  for (uint32_t k = 0; k < 4; ++k)
    r.links[radiosity_link_index(radiosity_slots(2), 0, k)] = RADIOSITY_NO_LINK;
  CHECK(r.solve(0.f, 5, F, &res) == 2 && F[0] == 1.f && F[1] == 1.5f); // (iteration 2 changes nothing: stop)
}

// ---- 2 ----
static void residual_order() {
  std::mt19937 gen(5);
  std::uniform_real_distribution<float> mag(-30.f, 10.f);
  for (int round = 0; round < 2000; ++round) {
    float fmaxv = 0.f;
    uint32_t bmax = 0;
    for (int i = 0; i < 64; ++i) {
      const float now = std::exp2(mag(gen)), before = std::exp2(mag(gen));
      const uint32_t b = radiosity_residual_bits(now, before);
      CHECK(radiosity_residual_value(b) == std::fabs(now - before));
      bmax = std::max(bmax, b);
      fmaxv = std::fmax(fmaxv, std::fabs(now - before));
    }
    CHECK(radiosity_residual_value(bmax) == fmaxv);
  }
  CHECK(radiosity_residual_bits(1.f, 1.f) == 0u && radiosity_residual_bits(0.f, 1.f) == bits(1.f));
  CHECK(radiosity_residual_bits(1.f, 1.5f) == bits(0.5f)); // the sign is dropped (-0.5)
  CHECK(radiosity_stops(0u, 0.f) && !radiosity_stops(1u, 0.f) && radiosity_stops(bits(1e-4f), 1e-4f));
  CHECK(radiosity_rho_ok(0.f) && radiosity_rho_ok(1.f) && radiosity_rho_ok(-0.f) && !radiosity_rho_ok(1.0000001f) &&
        !radiosity_rho_ok(-1e-30f) && !radiosity_rho_ok(NAN) && !radiosity_rho_ok(INFINITY));
  CHECK(radiosity_emission(0.5f, 3.f) == 1.5f);
}

// ---- 3 ----
static void large_indices() {
  const uint32_t N = (1u << 20) + 3u, K = 4100;
  const uint64_t slots = radiosity_slots(N), count = radiosity_link_count(N, K);
  CHECK(slots % 64 == 0 && slots >= N && slots < (uint64_t)N + 64);
  CHECK(count == slots * K && count > (1ull << 32));
  CHECK(radiosity_link_index(slots, N - 1, K - 1) == count - 1 - (slots - N)); // the last entry a lane owns
  CHECK(radiosity_link_index(slots, 0, 0) == 0 && radiosity_link_index(slots, 1, 0) == 1 && radiosity_link_index(slots, 0, 1) == slots);
  std::mt19937_64 gen(11);
  std::vector<uint64_t> seen;
  std::vector<std::pair<uint32_t, uint32_t>> keys;
  for (int i = 0; i < 200000; ++i) {
    // corners and the far end on purpose, the rest at random
    uint32_t slot = (uint32_t)(gen() % N), k = (uint32_t)(gen() % K);
    if (i % 5 == 0)
      slot = N - 1 - (uint32_t)(i % 7);
    if (i % 3 == 0)
      k = K - 1 - (uint32_t)(i % 11);
    const uint64_t idx = radiosity_link_index(slots, slot, k);
    CHECK(idx < count);
    CHECK(idx % slots == slot && idx / slots == k); // (the inverse: injective)
    seen.push_back(idx);
    keys.emplace_back(slot, k);
  }
  std::sort(seen.begin(), seen.end());
  std::sort(keys.begin(), keys.end());
  const size_t distinctIdx = std::unique(seen.begin(), seen.end()) - seen.begin();
  const size_t distinctKeys = std::unique(keys.begin(), keys.end()) - keys.begin();
  CHECK(distinctIdx == distinctKeys);
  CHECK(radiosity_slots(0) == 0 && radiosity_slots(1) == 64 && radiosity_slots(64) == 64 && radiosity_slots(65) == 128);
  CHECK(radiosity_slots(0xFFFFFFFFu) == 0x100000000ull);
}

// ---- 4 ----
static void cuts() {
  const float wmax = gather_wmax(4096); // 1024
  const float e[4] = {2000.f, INFINITY, 1024.f, NAN};
  CHECK(wmax == 1024.f);
  CHECK(radiosity_link_q(0, e, wmax) == gather_q(1024.f, wmax) && radiosity_link_q(1, e, wmax) == gather_q(1024.f, wmax));
  CHECK(radiosity_link_q(2, e, wmax) == (int64_t)1024 << 40);
  CHECK(radiosity_link_q(3, e, wmax) == 0 && radiosity_link_q(RADIOSITY_NO_LINK, e, wmax) == 0);
  // a row of 4096 links at a huge emission: 4096 x 1024 x 2^40 = 2^62, no overflow, result 1024 + direct
  int64_t sum = 0;
  for (int k = 0; k < 4096; ++k)
    sum += radiosity_link_q(1, e, wmax);
  CHECK(sum == (int64_t)1 << 62);
  CHECK(radiosity_row_result(0, sum, 4096) == 1024.f);
  // a link's contribution is gather_q of the table's entry, whatever it is
  std::mt19937 gen(3);
  std::uniform_real_distribution<float> u(-1.f, 2000.f);
  for (int i = 0; i < 100000; ++i) {
    const float v = u(gen);
    CHECK(radiosity_link_q(0, &v, wmax) == gather_q(v, wmax));
  }
}

int main() {
  two_facing_primitives();
  residual_order();
  large_indices();
  cuts();
  std::printf("%ld checks\n%ld failed checks\n", checks, failed);
  return failed ? 1 : 0;
}
