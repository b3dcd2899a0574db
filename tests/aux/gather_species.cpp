// The per-species step of the species gather (viennaray_amd/csrc/vr_gather.hpp: gather_species_absorb,
// gather_species_reflect, gather_species_step) on the host, stand-alone: this file includes vr_gather.hpp alone, the text
// the kernel compiles.  10^4 random paths of up to 12 vertices for NS = 2 and NS = 4: per vertex a reflectivity per species
// (zeros among them), a cosine mu, per species a reflectivity law or none (zeros among their entries).  Every species'
// throughput after every vertex, and the vertex it dies at, must be those of the single-species functions
// gather_path_throughput / gather_path_throughput_law walked alone, bit for bit; the mask must be empty exactly when every
// species is dead; a dead species' T is never touched again; the halves called as the kernel calls them and the combined
// step agree.  Prints "<n> checks" and "<m> failed checks".
#include "vr_gather.hpp"

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
static void check(bool ok, const char *what, int trial, int s, int v) {
  ++checks;
  if (!ok) {
    if (++failed <= 20)
      std::printf("FAILED %s: trial %d species %d vertex %d\n", what, trial, s, v);
  }
}
static bool same(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

constexpr int VERTS = 12;

template <int NS> static void trial(int id) {
  float rho[VERTS][NS], mu[VERTS], R[NS][GATHER_LAW_MAX];
  uint32_t MR[NS];
  const float *Rp[NS];
  for (int s = 0; s < NS; ++s) {
    const unsigned kind = (unsigned)(next64() % 4);
    MR[s] = kind == 0 ? 0u : (kind == 1 ? 2u : (kind == 2 ? 256u : 2u + (uint32_t)(next64() % 255)));
    for (uint32_t k = 0; k < GATHER_LAW_MAX; ++k)
      R[s][k] = next64() % 16 == 0 ? 0.f : uniform();
    if (next64() % 8 == 0) // a law that kills at every angle
      for (uint32_t k = 0; k < GATHER_LAW_MAX; ++k)
        R[s][k] = 0.f;
    Rp[s] = R[s];
  }
  for (int v = 0; v < VERTS; ++v) {
    const unsigned m = (unsigned)(next64() % 8);
    mu[v] = m == 0 ? 0.f : (m == 1 ? 1.f : (m == 2 ? -0.25f : uniform()));
    for (int s = 0; s < NS; ++s) {
      const unsigned r = (unsigned)(next64() % 10);
      rho[v][s] = r == 0 ? 0.f : (r == 1 ? 1.f : (r == 2 ? 1e-30f : uniform())); // (1e-30: the product underflows to 0 in two steps)
    }
  }
  // every species alone: T after vertex v, and the vertex it dies at (VERTS: never)
  float Tone[NS][VERTS];
  int death[NS];
  for (int s = 0; s < NS; ++s) {
    float T = 1.f;
    death[s] = VERTS;
    for (int v = 0; v < VERTS; ++v) {
      Tone[s][v] = 0.f;
      if (death[s] < VERTS)
        continue;
      T = gather_path_throughput(T, rho[v][s]);
      if (T != 0.f && MR[s])
        T = gather_path_throughput_law(T, R[s], MR[s], mu[v]);
      Tone[s][v] = T;
      if (T == 0.f)
        death[s] = v;
    }
  }
  // together: the halves as the kernel calls them, and the combined step beside them
  float T[NS], T2[NS], Tdead[NS];
  unsigned alive = (1u << NS) - 1u, alive2 = alive;
  for (int s = 0; s < NS; ++s)
    T[s] = T2[s] = 1.f, Tdead[s] = 0.f;
  for (int v = 0; v < VERTS && alive; ++v) {
    const unsigned before = alive;
    alive = gather_species_absorb<NS>(T, alive, rho[v]);
    if (alive)
      alive = gather_species_reflect<NS>(T, alive, Rp, MR, mu[v]);
    alive2 = gather_species_step<NS>(T2, alive2, rho[v], Rp, MR, mu[v]);
    check(alive == alive2, "the halves and the step give one mask", id, -1, v);
    bool anyAlive = false;
    for (int s = 0; s < NS; ++s) {
      const bool was = (before >> s) & 1u, is = (alive >> s) & 1u;
      check(was == (death[s] >= v), "alive before the vertex", id, s, v);
      check(is == (death[s] > v), "alive after the vertex", id, s, v);
      if (is) {
        check(same(T[s], Tone[s][v]) && T[s] != 0.f, "a living species' T is the single path's", id, s, v);
        check(same(T2[s], T[s]), "the step's T is the halves'", id, s, v);
      } else if (was) {
        // (killed by its rho the law is not applied; killed by the law T is 0 too: either way the single path's 0 here)
        check(T[s] == 0.f && Tone[s][v] == 0.f, "a species dies on a T of 0, where the single path dies", id, s, v);
        Tdead[s] = T[s];
      } else {
        check(same(T[s], Tdead[s]), "a dead species' T is not touched", id, s, v);
      }
      anyAlive = anyAlive || death[s] > v;
    }
    check((alive == 0u) == !anyAlive, "the mask is empty exactly when every species is dead", id, -1, v);
  }
}

int main() {
  for (int t = 0; t < 10000; ++t) {
    trial<2>(t);
    trial<4>(t);
  }
  // a species that is not in the mask from the start (three species in the four-wide kernel) is never touched
  {
    float T[4] = {1.f, 1.f, 1.f, 1.f};
    const float rho[4] = {0.5f, 0.25f, 1.f, 0.f};
    const float law[2] = {0.5f, 0.5f};
    const float *R[4] = {law, law, law, law};
    const uint32_t MR[4] = {2u, 0u, 2u, 2u};
    const unsigned alive = gather_species_step<4>(T, 7u, rho, R, MR, 0.3f);
    check(alive == 7u && T[0] == 0.25f && T[1] == 0.25f && T[2] == 0.5f && T[3] == 1.f, "a species outside the mask", 0, 3, 0);
  }
  std::printf("%ld checks\n%ld failed checks\n", checks, failed);
  return failed ? 1 : 0;
}
