// The catalogue of trace kernels (vr_types.hpp: mode_traits, trace_kernel_exists, trace_kernel_particle) on the host: prints
// it — one line per mode's traits, per kernel (with its mangled name) and per (particle, mode) request's serving particle
// id — and checks the counts of the sets and the invariants of the traits.  tests/test_kernel_catalogue_host.py reads the
// lines.  Plain C++17, vr_types.hpp alone.
#include <cstdio>
#include <initializer_list>

#include "vr_types.hpp"

using namespace vr;

static int failed = 0;
#define CHECK(cond)                                                                                                    \
  do {                                                                                                                 \
    if (!(cond)) {                                                                                                     \
      ++failed;                                                                                                        \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);                                                   \
    }                                                                                                                  \
  } while (0)

// both are usable where the kernel and the tables use them: in constant expressions
static_assert(mode_traits(MODE_ABSORB_FLAT_PLANAR_ROUND).base == MODE_ABSORB_FLAT && mode_traits(MODE_SMALL).dynamicLds, "");
static_assert(trace_kernel_exists(KERNELS_LIBRARY, 3, 0, 0, MODE_ABSORB_FLAT_UNIFORM) &&
                  !trace_kernel_exists(KERNELS_LIBRARY, 2, 0, 0, MODE_ABSORB_FLAT_UNIFORM), "");
static_assert(mode_traits(MODE_ABSORB_FLAT_LATTICE).base == MODE_ABSORB_FLAT && mode_traits(MODE_ABSORB_FLAT_LATTICE_LANES).base == MODE_ABSORB_FLAT, "");
static_assert(VR_NUM_MODES == 13, "");

// the kernels of `set` under particle ids lo .. hi, printed; returns their number
static int print_set(const char *name, KernelSet set, int lo, int hi) {
  int n = 0;
  for (int D = 2; D <= 3; ++D)
    for (int geo = 0; geo <= 1; ++geo)
      for (int particle = lo; particle <= hi; ++particle)
        for (int mode = 0; mode < VR_NUM_MODES; ++mode)
          if (trace_kernel_exists(set, D, geo, particle, mode)) {
            std::printf("kernel %s %d %d %d %d _ZN2vr12trace_kernelILi%dELi%dELi%dELi%dEEEvNS_11TraceParamsE\n", name, D, geo, particle,
                        mode, D, geo, particle, mode);
            ++n;
          }
  std::printf("count %s %d\n", name, n);
  return n;
}

int main() {
  for (int mode = 0; mode < VR_NUM_MODES; ++mode) {
    const ModeTraits t = mode_traits(mode);
    std::printf("mode %d base %d small %d relief %d resume %d uniform %d planar %d planarRound %d lattice %d latticeLanes %d waves %d absorbing %d "
                "multiQueue %d xcdQueues %d spanBins %d dynamicLds %d\n",
                mode, t.base, (int)t.small, (int)t.relief, (int)t.resume, (int)t.uniform, (int)t.planar, (int)t.planarRound,
                (int)t.lattice, (int)t.latticeLanes, t.waves,
                (int)t.absorbing, (int)t.multiQueue, (int)t.xcdQueues, t.spanBins, (int)t.dynamicLds);
    CHECK(t.base >= MODE_GENERAL && t.base <= MODE_GENERAL_FLAT);
    CHECK(mode_traits(t.base).base == t.base); // (a base mode is its own)
    CHECK(!t.latticeLanes || t.lattice);
    CHECK(!t.lattice || t.planarRound);
    CHECK(!t.planarRound || t.planar);
    CHECK(!t.planar || t.uniform);
    CHECK(!t.uniform || t.base == MODE_ABSORB_FLAT);
    CHECK(t.waves >= 1 && t.waves <= 8);
    CHECK(t.multiQueue == (t.base == MODE_GENERAL_FLAT)); // the kernel's MULTIQ
    CHECK(t.xcdQueues == (mode == MODE_GENERAL_FLAT));    // the host's rule is narrower ...
    CHECK(!t.xcdQueues || t.multiQueue);                  // ... and asks only of a kernel that reads the queue count
    CHECK(t.absorbing == (t.base == MODE_ABSORB_FLAT || t.base == MODE_ABSORB));
    CHECK(t.spanBins == 16 || t.spanBins == 32 || t.spanBins == 64);
    CHECK(t.dynamicLds == t.small && t.small == (mode == MODE_SMALL));
    CHECK(trace_dynamic_lds(mode, 4096u) == (mode == MODE_SMALL ? 4096u : 0u));
    for (int particle = 0; particle <= P_EXT_FULL_STATS; ++particle) {
      std::printf("served %d %d %d\n", particle, mode, trace_kernel_particle(particle, mode));
      CHECK(trace_kernel_particle(particle, mode) == (t.absorbing ? 0 : particle));
    }
  }
  for (int mode : {-1, (int)VR_NUM_MODES, 100}) { // not a mode: no traits, no kernel in any set
    CHECK(mode_traits(mode).base < 0);
    CHECK(!trace_kernel_exists(KERNELS_LIBRARY, 3, 0, 0, mode) && !trace_kernel_exists(KERNELS_MODULE, 3, 0, P_EXT, mode));
  }
  for (int mode = 0; mode < VR_NUM_MODES; ++mode) { // out of range: nothing
    CHECK(!trace_kernel_exists(KERNELS_LIBRARY, 1, 0, 0, mode) && !trace_kernel_exists(KERNELS_LIBRARY, 4, 0, 0, mode));
    CHECK(!trace_kernel_exists(KERNELS_LIBRARY, 3, 2, 0, mode) && !trace_kernel_exists(KERNELS_LIBRARY, 3, -1, 0, mode));
    CHECK(!trace_kernel_exists(KERNELS_LIBRARY, 3, 0, -1, mode) && !trace_kernel_exists(KERNELS_LIBRARY, 3, 0, P_EXT_FULL_STATS + 1, mode));
    CHECK(!trace_kernel_exists(KERNELS_MODULE, 3, 0, 0, mode) && !trace_kernel_exists(KERNELS_MODULE, 3, 0, 1, mode));
  }
  CHECK(print_set("library", KERNELS_LIBRARY, 0, P_EXT_FULL) == 67);
  CHECK(print_set("statistics", KERNELS_LIBRARY, P_EXT_STATS, P_EXT_FULL_STATS) == 18);
  CHECK(print_set("module_lean", KERNELS_MODULE, P_EXT, P_EXT) == 10);
  CHECK(print_set("module_full", KERNELS_MODULE, P_EXT_FULL, P_EXT_FULL) == 8);
  CHECK(print_set("module_lean_statistics", KERNELS_MODULE, P_EXT_STATS, P_EXT_STATS) == 10);
  CHECK(print_set("module_full_statistics", KERNELS_MODULE, P_EXT_FULL_STATS, P_EXT_FULL_STATS) == 8);
  std::printf("%d failed checks\n", failed);
  return failed ? 1 : 0;
}
