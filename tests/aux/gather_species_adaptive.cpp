// The rounds of the adaptive species gather (vr_gather_species_adaptive*) on the host, stand-alone: this file includes
// vr_gather.hpp alone, the text the kernels compile.  A synthetic "primitive" is a stream of up to 512 paths: per path a
// vertex count, per vertex a reflectivity per species (zeros among them) and a cosine, per species a reflectivity law or
// none and a weight at the source.  Every species is first run ALONE through the rounds of the adaptive gather — its own
// walk (gather_path_throughput, gather_path_throughput_law), its own two sums (gather_q, gather_q2), gather_converged under
// its own targets, gather_result and gather_stderr2 at the K it stops at.  Then all species run TOGETHER as the kernels run
// them: the shared walk (gather_species_absorb, gather_species_reflect) starts every path with alive = the primitive's
// mask, gather_species_decide gives the next mask and says who writes; the sums of a species that has left the mask are
// overwritten with rubbish, so a verdict that read them would show.  Every species' flux, stdErr and samplesUsed, the
// unconverged counts, totalSamples, rounds and walkedSamples must be those of the runs alone, bit for bit.
// Prints "<n> checks", "<m> failed checks" and what the streams covered.
#include "vr_gather.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>

using namespace vr;

static unsigned long long state = 0x9E3779B97F4A7C15ull;
static unsigned long long next64() {
  state ^= state << 13;
  state ^= state >> 7;
  state ^= state << 17;
  return state;
}
static float uniform() { return (float)(next64() >> 40) * 5.9604644775390625e-08f; } // [0, 1)

static long checks = 0, failed = 0;
static void check(bool ok, const char *what, int trial, int s) {
  ++checks;
  if (!ok) {
    if (++failed <= 20)
      std::printf("FAILED %s: trial %d species %d\n", what, trial, s);
  }
}
static bool same(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

constexpr int VERTS = 5, MAXK = 512, NSMAX = (int)GATHER_MAX_SPECIES;

struct Stream {
  int verts[MAXK];              // vertices of path k: where the shared geometry ends
  float rho[MAXK][VERTS][NSMAX]; // reflectivity of the primitive hit, per species
  float mu[MAXK][VERTS];
  float base[MAXK][NSMAX]; // the weight of species s at the source before its throughput
  float R[NSMAX][GATHER_LAW_MAX];
  uint32_t MR[NSMAX];
};
static Stream st;

struct Out {
  float flux = -1.f, stdErr = -1.f;
  uint32_t used = 0u, unconverged = 0u, rounds = 0u;
  uint64_t total = 0u;
};

// statistics of what the streams covered
static long streams = 0, stopsApart = 0, unconvergedSeen = 0, partialStarts = 0;
static long stopAt[16] = {0};

template <int NS> static void trial(int id, int S) {
  const uint32_t minSamples = 64u, maxSamples = 64u << (unsigned)(next64() % 4);
  const float wmax = gather_wmax(maxSamples);
  float rel[NSMAX] = {0.f, 0.f, 0.f, 0.f}, abs[NSMAX] = {0.f, 0.f, 0.f, 0.f};
  static const float RELS[6] = {0.f, 0.02f, 0.05f, 0.1f, 0.3f, 1.f}, ABSS[4] = {0.f, 0.f, 0.01f, 0.1f};
  float pBright[NSMAX];
  for (int s = 0; s < NS; ++s) {
    rel[s] = RELS[next64() % 6];
    abs[s] = ABSS[next64() % 4];
    pBright[s] = next64() % 6 == 0 ? 0.f : uniform(); // (0: a species in full shadow, converged at minSamples)
    const unsigned kind = (unsigned)(next64() % 4);
    st.MR[s] = kind == 0 ? 0u : (kind == 1 ? 2u : (kind == 2 ? 256u : 2u + (uint32_t)(next64() % 255)));
    for (uint32_t k = 0; k < GATHER_LAW_MAX; ++k)
      st.R[s][k] = next64() % 16 == 0 ? 0.f : uniform();
  }
  for (uint32_t k = 0; k < maxSamples; ++k) {
    st.verts[k] = (int)(next64() % (VERTS + 1));
    for (int v = 0; v < VERTS; ++v) {
      const unsigned m = (unsigned)(next64() % 8);
      st.mu[k][v] = m == 0 ? 0.f : (m == 1 ? 1.f : uniform());
      for (int s = 0; s < NS; ++s) {
        const unsigned r = (unsigned)(next64() % 10);
        st.rho[k][v][s] = r == 0 ? 0.f : (r == 1 ? 1.f : uniform());
      }
    }
    for (int s = 0; s < NS; ++s)
      st.base[k][s] = uniform() < pBright[s] ? (next64() % 64 == 0 ? 5000.f : 4.f * uniform()) : 0.f; // (5000: above wmax, above 2048)
  }
  // ---- every species alone ----
  Out one[NSMAX];
  for (int s = 0; s < S; ++s) {
    int64_t S1 = 0, S2 = 0;
    uint32_t K = 0u;
    for (uint32_t r = 0;; ++r) {
      const uint32_t first = r == 0 ? 0u : minSamples << (r - 1u), count = r == 0 ? minSamples : minSamples << (r - 1u);
      for (uint32_t k = first; k < first + count; ++k) {
        float T = 1.f;
        bool alive = true;
        for (int v = 0; v < st.verts[k] && alive; ++v) {
          T = gather_path_throughput(T, st.rho[k][v][s]);
          if (T != 0.f && st.MR[s])
            T = gather_path_throughput_law(T, st.R[s], st.MR[s], st.mu[k][v]);
          alive = T != 0.f;
        }
        const float w = alive ? st.base[k][s] * T : 0.f;
        S1 += gather_q(w, wmax);
        S2 += gather_q2(w, wmax);
      }
      K = first + count;
      one[s].total += count;
      ++one[s].rounds;
      const bool conv = gather_converged(S1, S2, K, rel[s], abs[s]);
      if (conv || K == maxSamples) {
        one[s].flux = gather_result(S1, K);
        one[s].stdErr = (float)std::sqrt(gather_stderr2(S1, S2, K));
        one[s].used = K;
        one[s].unconverged = conv ? 0u : 1u;
        break;
      }
    }
  }
  // ---- together: the host's round loop, the kernel's walk from the mask, the decide function ----
  Out all[NSMAX];
  int64_t S1[NSMAX] = {0, 0, 0, 0}, S2[NSMAX] = {0, 0, 0, 0};
  unsigned mask = (1u << S) - 1u;
  uint32_t rounds = 0u;
  uint64_t walked = 0u;
  for (uint32_t r = 0;; ++r) {
    const uint32_t first = r == 0 ? 0u : minSamples << (r - 1u), count = r == 0 ? minSamples : minSamples << (r - 1u);
    if (mask != (1u << S) - 1u)
      ++partialStarts;
    for (uint32_t k = first; k < first + count; ++k) {
      float T[NS];
      const float *Rp[NS];
      uint32_t MR[NS];
      for (int s = 0; s < NS; ++s)
        T[s] = 1.f, Rp[s] = st.R[s], MR[s] = st.MR[s];
      unsigned alive = mask; // (a species outside the mask is dead from the start)
      for (int v = 0; v < st.verts[k] && alive; ++v) {
        float rho[NS];
        for (int s = 0; s < NS; ++s)
          rho[s] = st.rho[k][v][s];
        alive = gather_species_absorb<NS>(T, alive, rho);
        if (alive)
          alive = gather_species_reflect<NS>(T, alive, Rp, MR, st.mu[k][v]);
      }
      for (int s = 0; s < NS; ++s)
        if ((alive >> s) & 1u) {
          const float w = st.base[k][s] * T[s];
          S1[s] += gather_q(w, wmax);
          S2[s] += gather_q2(w, wmax);
        }
    }
    const uint32_t K = first + count;
    ++rounds;
    walked += count;
    for (int s = 0; s < S; ++s)
      if ((mask >> s) & 1u)
        all[s].total += count;
    const bool last = K == maxSamples;
    unsigned writes = 0u;
    const unsigned next = gather_species_decide(S1, S2, (uint32_t)S, K, rel, abs, mask, last, writes);
    check((next & ~mask) == 0u && (writes & ~mask) == 0u, "the verdict stays inside the mask", id, -1);
    check(last ? writes == mask : writes == (mask & ~next), "who writes", id, -1);
    for (int s = 0; s < S; ++s) {
      if ((writes >> s) & 1u) {
        check(all[s].used == 0u, "a species writes once", id, s);
        all[s].flux = gather_result(S1[s], K);
        all[s].stdErr = (float)std::sqrt(gather_stderr2(S1[s], S2[s], K));
        all[s].used = K;
      }
      if (last && ((next >> s) & 1u))
        all[s].unconverged = 1u;
      if (((mask >> s) & 1u) && !((next >> s) & 1u) && !last) { // it has left: its sums are of an older K from now on
        S1[s] = 0x7000000000000000ll;
        S2[s] = -1;
      }
    }
    mask = next;
    if (last || mask == 0u)
      break;
  }
  // ---- the comparison ----
  uint32_t maxRounds = 0u;
  uint64_t maxUsed = 0u;
  bool apart = false;
  for (int s = 0; s < S; ++s) {
    ++streams;
    check(all[s].used == one[s].used, "samplesUsed", id, s);
    check(same(all[s].flux, one[s].flux), "flux", id, s);
    check(same(all[s].stdErr, one[s].stdErr), "stdErr", id, s);
    check(all[s].unconverged == one[s].unconverged, "unconverged", id, s);
    check(all[s].total == one[s].total && all[s].total == one[s].used, "totalSamples", id, s);
    maxRounds = one[s].rounds > maxRounds ? one[s].rounds : maxRounds;
    maxUsed = one[s].used > maxUsed ? one[s].used : maxUsed;
    apart = apart || one[s].used != one[0].used;
    unconvergedSeen += one[s].unconverged;
    for (int b = 0; b < 16; ++b)
      if (one[s].used == (64u << b))
        ++stopAt[b];
  }
  stopsApart += apart ? 1 : 0;
  check(rounds == maxRounds, "rounds is the maximum over the species", id, -1);
  check(walked == maxUsed, "walkedSamples is the largest samplesUsed", id, -1);
}

int main() {
  for (int t = 0; t < 4000; ++t) {
    const int S = 2 + (int)(next64() % 3);
    if (S == 2)
      trial<2>(t, S);
    else
      trial<4>(t, S);
  }
  // the verdict by hand: species 1 outside the mask is neither read nor written, "never" targets fail, the last round writes all
  {
    const int64_t S1[4] = {64ll << 40, 0x7000000000000000ll, 0, 0}, S2[4] = {64ll << 28, -1, 0, 0}; // species 0: 64 weights of 1
    const float rel[4] = {0.1f, 0.1f, 0.f, 0.1f}, abs[4] = {0.f, 0.f, 0.f, 0.f};
    unsigned writes = 99u;
    unsigned next = gather_species_decide(S1, S2, 4u, 64u, rel, abs, 0xDu, false, writes);
    check(next == 0x4u && writes == 0x9u, "species 0 and 3 converge, 2 never does, 1 is not looked at", 0, 1);
    next = gather_species_decide(S1, S2, 4u, 64u, rel, abs, 0xDu, true, writes);
    check(next == 0x4u && writes == 0xDu, "the last round writes the whole mask", 0, 1);
    next = gather_species_decide(S1, S2, 3u, 64u, rel, abs, 0x5u, false, writes);
    check(next == 0x4u && writes == 0x1u, "three species", 0, 2);
  }
  std::printf("%ld streams, %ld trials whose species stop at different K, %ld unconverged, %ld rounds started from a partial mask\n",
              streams, stopsApart, unconvergedSeen, partialStarts);
  std::printf("stops at K = 64, 128, 256, 512: %ld %ld %ld %ld\n", stopAt[0], stopAt[1], stopAt[2], stopAt[3]);
  check(streams >= 10000 && stopsApart > 100 && unconvergedSeen > 100 && partialStarts > 100, "the streams cover the mask path", -1, -1);
  check(stopAt[0] > 100 && stopAt[1] > 100 && stopAt[2] > 100 && stopAt[3] > 100, "every K is a stopping K", -1, -1);
  std::printf("%ld checks\n%ld failed checks\n", checks, failed);
  return failed ? 1 : 0;
}
