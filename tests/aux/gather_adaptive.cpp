// The arithmetic of the gather's second sum and standard error (viennaray_amd/csrc/vr_gather.hpp: gather_q2,
// gather_stderr2, gather_converged) on the host; tests/test_gather_adaptive_host.py builds and runs it, once plain and once
// under ASan + UBSan.  vr_gather.hpp is the only project header: the text the kernels compile.
//   (no argument)  the checks: gather_q2 against 128-bit integer arithmetic, the overflow bound for every power-of-two
//                  budget, gather_stderr2 / gather_converged against long double on hand-made sums.  Prints "<n> checks"
//                  and "<m> failed checks".
//   se2            reads "S1 S2 K" lines from stdin, prints gather_stderr2 as a hex double and the verdict of
//                  gather_converged(rel = 0.05, abs = 0) per line: what numpy float64 must reproduce bit for bit.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "vr_gather.hpp"

using namespace vr;

static long checks = 0, failed = 0;
#define CHECK(cond)                                                                                                    \
  do {                                                                                                                 \
    ++checks;                                                                                                          \
    if (!(cond)) {                                                                                                     \
      if (++failed < 20)                                                                                               \
        std::printf("FAILED line %d: %s\n", __LINE__, #cond);                                                          \
    }                                                                                                                  \
  } while (0)

// floor(wc^2 2^28 + 1/2) in integers: a positive float is m 2^e with a 24-bit m, so wc^2 2^28 = m^2 2^(2e + 28)
static int64_t q2_exact(float w, float wmax) {
  if (!(w > 0.f))
    return 0;
  float wc = w > wmax ? wmax : w;
  if (wc > 2048.f)
    wc = 2048.f;
  int e;
  const float fr = std::frexp(wc, &e);                   // wc = fr 2^e, fr in [0.5, 1)
  const unsigned __int128 m = (unsigned __int128)(uint64_t)std::ldexp((double)fr, 24); // exact: 24 bits
  const int shift = 2 * (e - 24) + 28;                   // wc^2 2^28 = m^2 2^shift
  const unsigned __int128 mm = m * m;
  if (shift >= 0)
    return (int64_t)(mm << shift); // (wc <= 2048: below 2^51)
  if (-shift >= 100)
    return 0;
  // round to nearest by adding a half and flooring, as the header does
  const unsigned __int128 half = (unsigned __int128)1 << (-shift - 1);
  return (int64_t)((mm + half) >> -shift);
}

static void check_q2() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float wmaxes[] = {4194304.f, 65536.f, 4096.f, 2048.f, 1024.f, 16.f, 1.f, 0.5f};
  for (float wmax : wmaxes) {
    CHECK(gather_q2(0.f, wmax) == 0 && gather_q2(-0.f, wmax) == 0 && gather_q2(-1.f, wmax) == 0 && gather_q2(-inf, wmax) == 0);
    CHECK(gather_q2(nan, wmax) == 0);
    CHECK(gather_q2(1e-45f, wmax) == 0 && gather_q2(1e-40f, wmax) == 0); // denormals: far below half a unit
    if (wmax >= 1.f)
      CHECK(gather_q2(1.f, wmax) == ((int64_t)1 << 28));
    CHECK(gather_q2(inf, wmax) == q2_exact(wmax, wmax));
    CHECK(gather_q2(wmax * 2.f, wmax) == gather_q2(wmax, wmax));
    // the wmax and 2048 boundaries: the floats next to them
    const float edges[] = {wmax, std::nextafter(wmax, 0.f), std::nextafter(wmax, inf), 2048.f, std::nextafter(2048.f, 0.f),
                           std::nextafter(2048.f, inf)};
    for (float w : edges)
      CHECK(gather_q2(w, wmax) == q2_exact(w, wmax));
    // g values: g_3(n) = (n + 1) / 2 and g_2(n) for some powers
    for (float n : {1.f, 2.f, 3.f, 8.f, 100.f, 1000.f})
      for (int D : {2, 3}) {
        const float g = gather_g(n, D);
        CHECK(gather_q2(g, wmax) == q2_exact(g, wmax));
      }
    // a sweep over the exponents and mantissas
    uint32_t x = 12345u;
    for (int i = 0; i < 40000; ++i) {
      x = x * 1664525u + 1013904223u;
      const int e = (int)(x >> 26) - 40; // 2^-40 .. 2^23
      x = x * 1664525u + 1013904223u;
      const float w = std::ldexp(1.f + (float)(x >> 9) * 1.1920929e-07f, e);
      CHECK(gather_q2(w, wmax) == q2_exact(w, wmax));
    }
  }
  CHECK(gather_q2(1.f, 1024.f) == 268435456);
  // a weight of 1 squares to sum >> 12: q(1) = 2^40
  CHECK((gather_q(1.f, 1024.f) >> 12) == gather_q2(1.f, 1024.f));
}

// budget x q2(wmax(budget)) for every power-of-two budget the gather accepts (samples x g <= 2^22, g >= 1)
static void check_overflow() {
  for (int b = 0; b <= 22; ++b) {
    const uint32_t budget = 1u << b;
    const float wmax = gather_wmax(budget);
    const unsigned __int128 worst = (unsigned __int128)budget * (unsigned __int128)gather_q2(wmax, wmax);
    CHECK(worst < ((unsigned __int128)1 << 62));
    CHECK(worst <= ((unsigned __int128)1 << 61));
    CHECK(gather_q2(std::numeric_limits<float>::infinity(), wmax) == gather_q2(wmax, wmax));
    if (b > 0) { // a budget that is no power of two has the wmax of the next one
      const uint32_t odd = budget - (budget > 2 ? 1u : 0u);
      CHECK((unsigned __int128)odd * (unsigned __int128)gather_q2(1e30f, gather_wmax(odd)) <= ((unsigned __int128)1 << 61));
    }
  }
}

static long double se2_ld(int64_t S1, int64_t S2, uint32_t K, long double &m1) {
  m1 = (long double)S1 / 1099511627776.0L / K;
  const long double m2 = (long double)S2 / 268435456.0L / K;
  long double v = m2 - m1 * m1;
  if (!(v > 0))
    v = 0;
  return v / (K - 1);
}
static bool close(double a, long double b) {
  const long double d = fabsl((long double)a - b);
  return d <= 1e-13L * fabsl(b) + 1e-300L;
}

static void check_stderr() {
  // all-equal weights: K samples of w = 1, 0.5, 2, g_3(3) = 2 — m2 == m1^2 exactly, se2 exactly 0
  for (float w : {1.f, 0.5f, 2.f, 0.25f, 1024.f})
    for (uint32_t K : {64u, 128u, 1024u, 4096u}) {
      const int64_t S1 = (int64_t)K * gather_q(w, 4096.f), S2 = (int64_t)K * gather_q2(w, 4096.f);
      CHECK(gather_stderr2(S1, S2, K) == 0.);
      CHECK(gather_converged(S1, S2, K, 0.05f, 0.f));
      CHECK(gather_converged(S1, S2, K, 0.f, 1e-30f));
      CHECK(!gather_converged(S1, S2, K, 0.f, 0.f)); // "never"
    }
  // nothing seen: converged under any positive target
  CHECK(gather_stderr2(0, 0, 64) == 0. && gather_converged(0, 0, 64, 0.05f, 0.f) && gather_converged(0, 0, 64, 0.f, 1e-3f));
  CHECK(!gather_converged(0, 0, 64, 0.f, 0.f));
  // two values: a samples of 1 and K - a of 0 — mean p = a / K, variance p (1 - p), se2 = p (1 - p) / (K - 1)
  for (uint32_t K : {64u, 256u, 4096u})
    for (uint32_t a = 1; a < K; a += (K / 16u) | 1u) {
      const int64_t S1 = (int64_t)a << 40, S2 = (int64_t)a << 28;
      const double p = (double)a / K, want = p * (1. - p) / (K - 1.);
      const double got = gather_stderr2(S1, S2, K);
      CHECK(std::fabs(got - want) <= 1e-15 * want + 1e-18);
      long double m1;
      CHECK(close(got, se2_ld(S1, S2, K, m1)) || std::fabs(got - (double)se2_ld(S1, S2, K, m1)) <= 1e-17);
      // the rule: se2 <= (rel m1)^2
      const float rel = 0.05f;
      const long double tol = (long double)rel * m1;
      const long double margin = fabsl(se2_ld(S1, S2, K, m1) - tol * tol);
      if (margin > 1e-12L * tol * tol)
        CHECK(gather_converged(S1, S2, K, rel, 0.f) == (se2_ld(S1, S2, K, m1) <= tol * tol));
      // an absolute target above and below the error
      const float se = (float)std::sqrt(got);
      CHECK(gather_converged(S1, S2, K, 0.f, se * 1.01f) && !gather_converged(S1, S2, K, 0.f, se * 0.99f));
    }
  // two values 1 and 3, half each: mean 2, variance 1
  {
    const uint32_t K = 128;
    const int64_t S1 = 64 * gather_q(1.f, 4096.f) + 64 * gather_q(3.f, 4096.f);
    const int64_t S2 = 64 * gather_q2(1.f, 4096.f) + 64 * gather_q2(3.f, 4096.f);
    CHECK(gather_stderr2(S1, S2, K) == 1. / 127.);
  }
  // v < 0 by rounding: the squares are quantised at 2^-28, the mean at 2^-40 — equal weights w whose square rounds DOWN
  // give m2 < m1^2; se2 is 0, not negative and not NaN
  long neg = 0;
  uint32_t x = 99u;
  for (int i = 0; i < 20000; ++i) {
    x = x * 1664525u + 1013904223u;
    const float w = 0.001f + (float)(x >> 8) * 5.9604645e-08f;
    const uint32_t K = 64u << (x & 3u);
    const int64_t S1 = (int64_t)K * gather_q(w, 4096.f), S2 = (int64_t)K * gather_q2(w, 4096.f);
    long double m1;
    const long double m2 = (long double)S2 / 268435456.0L / K;
    (void)se2_ld(S1, S2, K, m1);
    const double se2 = gather_stderr2(S1, S2, K);
    CHECK(se2 >= 0. && se2 <= 1e-9);
    if (m2 < m1 * m1 * (1 - 1e-12L)) {
      ++neg;
      CHECK(se2 == 0.);
      CHECK(gather_converged(S1, S2, K, 0.05f, 0.f));
    }
  }
  CHECK(neg > 1000);
  // random sums against long double
  for (int i = 0; i < 50000; ++i) {
    x = x * 1664525u + 1013904223u;
    const uint32_t K = 64u * (1u + (x >> 27));
    x = x * 1664525u + 1013904223u;
    const uint32_t a = x % (K + 1u);
    x = x * 1664525u + 1013904223u;
    const float w = 0.01f + (float)(x >> 8) * 1.1920929e-07f * 4.f; // a samples of w, the rest 0
    const int64_t S1 = (int64_t)a * gather_q(w, 1024.f), S2 = (int64_t)a * gather_q2(w, 1024.f);
    long double m1;
    const long double ref = se2_ld(S1, S2, K, m1);
    const double got = gather_stderr2(S1, S2, K);
    // (v = m2 - m1^2 cancels: the double result is within a few ulp of m2 / (K - 1) of the long double one)
    CHECK(fabsl((long double)got - ref) <= 1e-15L * (long double)S2 / 268435456.0L / K);
  }
}

int main(int argc, char **argv) {
  if (argc > 1 && !std::strcmp(argv[1], "se2")) {
    long long S1, S2;
    unsigned K;
    while (std::scanf("%lld %lld %u", &S1, &S2, &K) == 3)
      std::printf("%a %d\n", gather_stderr2(S1, S2, K), gather_converged(S1, S2, K, 0.05f, 0.f) ? 1 : 0);
    return 0;
  }
  check_q2();
  check_overflow();
  check_stderr();
  std::printf("%ld checks\n%ld failed checks\n", checks, failed);
  return failed ? 1 : 0;
}
