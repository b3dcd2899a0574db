// The per-ray bookkeeping of castRays (viennaray_amd/csrc/vr_cast.hpp) on the host: the header the kernel includes, taken
// by the host compiler alone.  A table of segment sequences against the expected (prim, dist, boundaryHits, has a point),
// then random chains: the tmax rule — a bounded cast is the unbounded one with everything beyond tmax turned into a miss —
// and that dist never decreases.  Prints "<n> failed checks"; exit status 1 if any.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "vr_cast.hpp"

using namespace vr;

static const float INF = std::numeric_limits<float>::infinity();

struct Seg {
  int geom;      // -1 miss, 0 wall, 1 geometry
  uint32_t prim; // wall or primitive id
  float t;
  bool ignore;   // a wall whose boundary condition is IGNORE
};

struct Out {
  int32_t prim;
  float dist;
  uint32_t bh;
  bool hit;
  size_t used; // segments consumed
};

// the kernel's loop (vr_cast.hip) over a prescribed chain of segments; a chain that runs out ends in a miss
static Out run(const std::vector<Seg> &segs, bool follow, uint32_t maxBh, float tmax, bool *monotone = nullptr) {
  CastState s;
  cast_begin(s);
  size_t k = 0;
  bool active = true;
  while (active) {
    const Seg seg = k < segs.size() ? segs[k] : Seg{-1, 0u, 0.f, false};
    ++k;
    const float before = s.dist;
    if (cast_segment(s, seg.geom, seg.prim, seg.t, follow, maxBh, tmax) == CAST_AT_WALL) {
      if (seg.ignore) {
        cast_ignored(s);
        active = false;
      }
    } else {
      active = false;
    }
    if (monotone && !(s.dist >= before))
      *monotone = false;
  }
  Out o{};
  cast_finish(s, tmax, o.prim, o.dist, o.bh, o.hit);
  o.used = k;
  return o;
}

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

static long failed = 0;
static void expect(const char *what, const Out &got, int32_t prim, float dist, uint32_t bh, bool hit, size_t used) {
  if (got.prim != prim || !same_bits(got.dist, dist) || got.bh != bh || got.hit != hit || got.used != used) {
    ++failed;
    std::printf("FAILED %s: got (%d, %a, %u, %d, used %zu) expected (%d, %a, %u, %d, used %zu)\n", what, got.prim, got.dist,
                got.bh, (int)got.hit, got.used, prim, dist, bh, (int)hit, used);
  }
}

// the float32 sum in segment order, as the definition has it
static float fsum(std::initializer_list<float> ts) {
  volatile float s = 0.f;
  for (float t : ts)
    s = s + t;
  return s;
}

int main() {
  long cases = 0;
  const Seg G7{1, 7u, 2.5f, false}, W2{0, 2u, 1.25f, false}, W5{0, 5u, 0.1f, false}, WI{0, 3u, 0.75f, true}, MISS{-1, 0u, 0.f, false};
  // ---- one segment ----
  expect("geometry", run({G7}, true, 1000u, INF), 7, 2.5f, 0u, true, 1), ++cases;
  expect("geometry, not following", run({G7}, false, 1000u, INF), 7, 2.5f, 0u, true, 1), ++cases;
  expect("miss", run({MISS}, true, 1000u, INF), CAST_MISS, INF, 0u, false, 1), ++cases;
  expect("wall, not following", run({W2, G7}, false, 1000u, INF), CAST_WALL, 1.25f, 0u, true, 1), ++cases;
  expect("primitive 0 is a hit", run({Seg{1, 0u, 1.f, false}}, true, 1000u, INF), 0, 1.f, 0u, true, 1), ++cases;
  expect("t = 0", run({Seg{1, 3u, 0.f, false}}, true, 1000u, 0.f), 3, 0.f, 0u, true, 1), ++cases;
  // ---- chains ----
  expect("wall then geometry", run({W2, G7}, true, 1000u, INF), 7, fsum({1.25f, 2.5f}), 1u, true, 2), ++cases;
  expect("two walls then geometry", run({W2, W5, G7}, true, 1000u, INF), 7, fsum({1.25f, 0.1f, 2.5f}), 2u, true, 3), ++cases;
  expect("wall then miss keeps the count", run({W2, MISS}, true, 1000u, INF), CAST_MISS, INF, 1u, false, 2), ++cases;
  expect("ignore wall", run({WI, G7}, true, 1000u, INF), CAST_MISS, INF, 0u, false, 1), ++cases;
  expect("wall, ignore wall", run({W2, WI, G7}, true, 1000u, INF), CAST_MISS, INF, 1u, false, 2), ++cases;
  // ---- the budget: the tracer's ++boundaryHits > maxBoundaryHits ----
  expect("budget 0 stops on the first wall", run({W2, G7}, true, 0u, INF), CAST_WALL, 1.25f, 0u, true, 1), ++cases;
  expect("budget 1 passes one wall", run({W2, G7}, true, 1u, INF), 7, fsum({1.25f, 2.5f}), 1u, true, 2), ++cases;
  expect("budget 1 stops on the second", run({W2, W5, G7}, true, 1u, INF), CAST_WALL, fsum({1.25f, 0.1f}), 1u, true, 2), ++cases;
  expect("budget 3, four walls", run({W2, W5, W2, W5, G7}, true, 3u, INF), CAST_WALL, fsum({1.25f, 0.1f, 1.25f, 0.1f}), 3u, true, 4),
      ++cases;
  expect("an ignore wall beyond the budget is a wall", run({W2, WI}, true, 1u, INF), CAST_WALL, fsum({1.25f, 0.75f}), 1u, true, 2),
      ++cases;
  expect("no budget at all", run({W2, W5, G7}, true, 0xFFFFFFFFu, INF), 7, fsum({1.25f, 0.1f, 2.5f}), 2u, true, 3), ++cases;
  // ---- tmax ----
  expect("hit at exactly tmax counts", run({G7}, true, 1000u, 2.5f), 7, 2.5f, 0u, true, 1), ++cases;
  expect("hit beyond tmax", run({G7}, true, 1000u, std::nextafterf(2.5f, 0.f)), CAST_MISS, INF, 0u, false, 1), ++cases;
  expect("tmax 0 misses", run({G7}, true, 1000u, 0.f), CAST_MISS, INF, 0u, false, 1), ++cases;
  expect("chain at exactly tmax", run({W2, G7}, true, 1000u, fsum({1.25f, 2.5f})), 7, fsum({1.25f, 2.5f}), 1u, true, 2), ++cases;
  expect("chain stopped at the wall beyond tmax", run({W2, W5, G7}, true, 1000u, 1.3f), CAST_MISS, INF, 0u, false, 2), ++cases;
  expect("wall beyond tmax, not following", run({W2}, false, 1000u, 1.f), CAST_MISS, INF, 0u, false, 1), ++cases;
  expect("wall at tmax, not following", run({W2}, false, 1000u, 1.25f), CAST_WALL, 1.25f, 0u, true, 1), ++cases;
  expect("a miss under a finite tmax reports no walls", run({W2, MISS}, true, 1000u, 100.f), CAST_MISS, INF, 0u, false, 2), ++cases;
  expect("infinite segment", run({Seg{1, 4u, INF, false}}, true, 1000u, INF), 4, INF, 0u, true, 1), ++cases;

  // ---- random chains: bounded = unbounded with everything beyond tmax turned into a miss; dist never decreases ----
  std::mt19937 rng(20240u);
  const float ts[] = {0.f, 1e-4f, 1e-3f, 0.1f, 0.3f, 1.f, 1.25f, 7.f, 1e3f, 3e7f, 1e-30f};
  long chains = 0, bounded_hits = 0, bounded_misses = 0, exact = 0;
  for (int it = 0; it < 200000; ++it) {
    std::vector<Seg> segs;
    const int len = 1 + (int)(rng() % 6u);
    for (int k = 0; k < len; ++k) {
      const unsigned r = rng() % 10u;
      const float t = ts[rng() % (sizeof(ts) / sizeof(ts[0]))];
      if (r < 6u)
        segs.push_back(Seg{0, (uint32_t)(rng() % 8u), t, rng() % 12u == 0u});
      else if (r < 9u)
        segs.push_back(Seg{1, (uint32_t)(rng() % 1000u), t, false});
      else
        segs.push_back(MISS);
    }
    const bool follow = rng() % 4u != 0u;
    const uint32_t maxBh = rng() % 5u;
    bool mono = true;
    const Out u = run(segs, follow, maxBh, INF, &mono);
    // tmax: one of the chain's own partial sums (so that "exactly tmax" is met), or a value from the table
    float tmax = ts[rng() % (sizeof(ts) / sizeof(ts[0]))];
    if (rng() % 2u) {
      volatile float s = 0.f;
      const size_t upto = 1 + rng() % segs.size();
      for (size_t k = 0; k < upto; ++k)
        s = s + (segs[k].geom >= 0 ? segs[k].t : 0.f);
      tmax = s;
    }
    const Out b = run(segs, follow, maxBh, tmax, &mono);
    Out want = u;
    if (u.dist > tmax) { // (a miss has dist +inf: beyond every finite tmax)
      want.prim = CAST_MISS;
      want.dist = INF;
      want.hit = false;
    }
    if (want.prim == CAST_MISS)
      want.bh = 0u;
    ++chains;
    bounded_hits += b.prim != CAST_MISS;
    bounded_misses += b.prim == CAST_MISS && u.prim != CAST_MISS;
    exact += b.prim != CAST_MISS && same_bits(b.dist, tmax);
    if (!mono || b.prim != want.prim || !same_bits(b.dist, want.dist) || b.bh != want.bh || b.hit != want.hit || b.used > u.used) {
      ++failed;
      if (failed < 10)
        std::printf("FAILED chain %d: bounded (%d, %a, %u, %d) expected (%d, %a, %u, %d) tmax %a monotone %d\n", it, b.prim, b.dist,
                    b.bh, (int)b.hit, want.prim, want.dist, want.bh, (int)want.hit, tmax, (int)mono);
    }
  }
  std::printf("%ld table cases, %ld random chains: %ld bounded results kept, %ld turned into a miss, %ld kept at exactly tmax\n",
              cases, chains, bounded_hits, bounded_misses, exact);
  std::printf("%ld failed checks\n", failed);
  return failed ? 1 : 0;
}
