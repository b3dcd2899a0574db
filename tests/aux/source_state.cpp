// source_state.cpp — RaySource (viennaray_amd/csrc/vr_source.hpp) alone, on the CPU: from each of the five kinds every
// setter and every clearing call; after each step the kind, the payload of the kind in force (what the setter was given),
// the payload of every other kind (empty), sourceDirty, the ray count with numRaysFixed unset and set, and the answers of
// the named questions against the tables written out below — which are the behaviour of the expressions these questions
// replaced.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>
#include <vector>

#include "../../viennaray_amd/csrc/vr_source.hpp"

using namespace vr;

static int failures = 0;
#define CHECK(cond, what)                                                                                              \
  do {                                                                                                                 \
    if (!(cond)) {                                                                                                     \
      std::printf("FAILED %s: %s (line %d)\n", (what).c_str(), #cond, __LINE__);                                       \
      ++failures;                                                                                                      \
    }                                                                                                                  \
  } while (0)

// the states a source can be in, as far as any question can tell them apart
enum State { R, G, H, HW, S, M, MW, NUM_STATES };
static const char *const kStateName[NUM_STATES] = {"Random", "Grid", "HostRays", "HostRays+weights", "Surface", "Model", "Model+kHasWeight"};
static const SourceKind kKindOf[NUM_STATES] = {SourceKind::Random, SourceKind::Grid, SourceKind::HostRays, SourceKind::HostRays,
                                               SourceKind::Surface, SourceKind::Model, SourceKind::Model};

// The answers, by state.  `primary`: SourceRandom's primary direction is set (it may be, under any source).
struct Answers {
  bool weighted;       // no absorbing kernel:        (host rays && weights) || surface || model with kHasWeight
  bool genWeights;     // the generator writes them:  surface || model with kHasWeight
  bool side[2];        // records' side array, a particle that goes on, [primary]:
                       //                             primary || grid || host rays || model || surface  (|| stateful)
  bool slabs[2];       // RNG slabs for the generator grid, [primary]:
                       //                             primary || host rays || model                     (|| stateful)
  bool plain[2];       // relief packets, [primary]:  !primary && !grid && !host rays && !model && !surface
  bool stateful;       // a stateful model may run:   !grid && !host rays && !model && !surface
  Generator gen[2];    // [primary]: surface ? 4 : host rays ? 3 : grid ? 2 : primary ? 1 : 0; a model: its module's
};
static const Answers kAnswers[NUM_STATES] = {
    /* R  */ {false, false, {false, true}, {false, true}, {true, false}, true, {GEN_RANDOM, GEN_BASIS}},
    /* G  */ {false, false, {true, true}, {false, true}, {false, false}, false, {GEN_GRID, GEN_GRID}},
    /* H  */ {false, false, {true, true}, {true, true}, {false, false}, false, {GEN_HOST, GEN_HOST}},
    /* HW */ {true, false, {true, true}, {true, true}, {false, false}, false, {GEN_HOST, GEN_HOST}},
    /* S  */ {true, true, {true, true}, {false, true}, {false, false}, false, {GEN_SURFACE, GEN_SURFACE}},
    /* M  */ {false, false, {true, true}, {true, true}, {false, false}, false, {GEN_SOURCE_MODEL, GEN_SOURCE_MODEL}},
    /* MW */ {true, true, {true, true}, {true, true}, {false, false}, false, {GEN_SOURCE_MODEL, GEN_SOURCE_MODEL}},
};

// the counts of an apply: 100 primitives, 10 rays per point; numRaysFixed unset, or 64
constexpr uint32_t PRIMS = 100;
constexpr uint64_t PER_POINT = 10, FIXED = 64;

// what the test knows about the state it has put the source in
struct Expect {
  State state = R;
  uint64_t points = 0;  // grid points / host rays / surface points
  uint64_t ownRays = 0; // a model's own ray count (0: SourceRandom's)
  bool draws = false;   // host rays with draw counts
  // the scalars the setter of the kind in force was given
  float area = 0.f, offset = 0.f;       // surface
  int32_t model = -1;                   // model: id, parameters given, table entries
  uint32_t nparams = 0, table = 0;
  bool dirty = false;   // sourceDirty: raised by every call of set_grid, set_host_rays and set_host_weights that is not
                        // refused (the clearing ones included), lowered by nobody here
};

// the payloads handed to the setters: every value differs from its neighbours and from the other arrays'
static std::vector<float> ramp(size_t n, float first) {
  std::vector<float> v(n);
  for (size_t k = 0; k < n; ++k)
    v[k] = first + (float)k;
  return v;
}
static const std::vector<float> kFloats = ramp(64, 0.5f), kDirs = ramp(64, 100.25f), kWeights = ramp(16, 1000.125f);
static const std::vector<uint32_t> kDraws = {3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8, 9, 7, 9, 3};
static const float kParams[3] = {0.25f, 0.5f, 0.75f};

static void check(const RaySource &s, const Expect &e, const std::string &what) {
  const Answers &a = kAnswers[e.state];
  CHECK(s.kind == kKindOf[e.state], what);
  // the payload: of the kind in force what was set, of every other kind nothing
  CHECK(s.gridPoints.size() == (e.state == G ? e.points * 3 : 0), what);
  CHECK(s.hostOrg.size() == ((e.state == H || e.state == HW) ? e.points * 3 : 0), what);
  CHECK(s.hostDir.size() == s.hostOrg.size(), what);
  CHECK(s.hostDraws.size() == (((e.state == H || e.state == HW) && e.draws) ? e.points : 0), what);
  CHECK(s.hostWeights.size() == (e.state == HW ? e.points : 0), what);
  CHECK(s.surfCount == (e.state == S ? e.points : 0), what);
  CHECK(s.sourceModel == ((e.state == M || e.state == MW) ? e.model : -1), what);
  CHECK(s.sourceDirty == e.dirty, what);
  // ... and of the kind in force the values, not only the sizes
  if (e.state == G)
    CHECK(std::equal(s.gridPoints.begin(), s.gridPoints.end(), kFloats.begin()), what);
  if (e.state == H || e.state == HW) {
    CHECK(std::equal(s.hostOrg.begin(), s.hostOrg.end(), kFloats.begin()), what);
    CHECK(std::equal(s.hostDir.begin(), s.hostDir.end(), kDirs.begin()), what);
    CHECK(std::equal(s.hostDraws.begin(), s.hostDraws.end(), kDraws.begin()), what);
    CHECK(std::equal(s.hostWeights.begin(), s.hostWeights.end(), kWeights.begin()), what);
  }
  if (e.state == S)
    CHECK(s.surfArea == e.area && s.surfOffset == e.offset, what);
  if (e.state == M || e.state == MW) {
    CHECK(s.srcHasWeight == (e.state == MW) && s.srcTableCount == e.table && s.srcNumRays == e.ownRays, what);
    for (uint32_t k = 0; k < (uint32_t)VR_SOURCE_PARAMS; ++k) // (zeros behind the parameters given)
      CHECK(s.srcParams[k] == (k < e.nparams ? kParams[k] : 0.f), what);
  }
  // the ray count, numRaysFixed unset and set
  uint64_t free = PRIMS * PER_POINT, fixed = FIXED;
  switch (e.state) {
  case R: break;
  case G: free = e.points * PER_POINT; break;
  case H:
  case HW: free = fixed = e.points; break;
  case S:
    free = e.points * PER_POINT;
    fixed = e.points * FIXED;
    break;
  case M:
  case MW:
    if (e.ownRays)
      free = fixed = e.ownRays;
    break;
  default: break;
  }
  CHECK(s.rays_of_apply(PRIMS, PER_POINT, 0) == free, what);
  CHECK(s.rays_of_apply(PRIMS, 0, FIXED) == fixed, what);
  // the questions
  CHECK(s.rays_start_weighted() == a.weighted, what);
  CHECK(s.generator_writes_weights() == a.genWeights, what);
  CHECK(s.admits_stateful_model() == a.stateful, what);
  for (int primary = 0; primary < 2; ++primary) {
    CHECK(s.records_carry_side_array(primary, false, false) == a.side[primary], what);
    CHECK(s.records_carry_side_array(primary, true, false), what);   // a stateful model's init draws first
    CHECK(!s.records_carry_side_array(primary, false, true), what);  // an absorbing launch reads no side array
    CHECK(!s.records_carry_side_array(primary, true, true), what);
    CHECK(s.generator_draws_past_tier1(primary, false) == a.slabs[primary], what);
    CHECK(s.generator_draws_past_tier1(primary, true), what);
    CHECK(s.is_plain(primary) == a.plain[primary], what);
    CHECK(s.generator(primary) == a.gen[primary], what);
  }
}

// ---- the steps ----------------------------------------------------------------------------------------------------
struct Step {
  const char *name;
  std::function<void(RaySource &, Expect &)> run; // applies the call and says what it must leave
};

static void to_random(Expect &e, bool dirty) {
  e = Expect{};
  e.dirty = dirty;
}

static const std::vector<Step> kSteps = {
    // the setters
    {"set_grid(7)", [](RaySource &s, Expect &e) {
       s.set_grid(kFloats.data(), 7);
       e = Expect{G, 7};
       e.dirty = true;
     }},
    {"set_host_rays(5, draws)", [](RaySource &s, Expect &e) {
       s.set_host_rays(kFloats.data(), kDirs.data(), kDraws.data(), 5);
       e = Expect{H, 5, 0, true}; // (new rays: no weights, whatever was there)
       e.dirty = true;
     }},
    {"set_host_rays(4, no draws)", [](RaySource &s, Expect &e) {
       s.set_host_rays(kFloats.data(), kDirs.data(), nullptr, 4);
       e = Expect{H, 4};
       e.dirty = true;
     }},
    {"set_surface(3)", [](RaySource &s, Expect &e) {
       const bool dirty = e.dirty;
       s.set_surface(3, 2.f, 1e-3f);
       e = Expect{S, 3};
       e.area = 2.f;
       e.offset = 1e-3f;
       e.dirty = dirty;
     }},
    {"set_model(no weight, SourceRandom's count)", [](RaySource &s, Expect &e) {
       const bool dirty = e.dirty;
       s.set_model(1, false, kParams, 3, 0, 0);
       e = Expect{M};
       e.model = 1;
       e.nparams = 3;
       e.dirty = dirty;
     }},
    {"set_model(kHasWeight, 11 rays, table)", [](RaySource &s, Expect &e) {
       const bool dirty = e.dirty;
       s.set_model(0, true, nullptr, 0, 5, 11);
       e = Expect{MW, 0, 11};
       e.model = 0;
       e.table = 5;
       e.dirty = dirty;
     }},
    // host-ray weights: one per host ray or refused — so any count is refused while host rays are not in force
    {"set_host_weights(6)", [](RaySource &s, Expect &e) {
       const bool hostRays = e.state == H || e.state == HW;
       const bool ok = s.set_host_weights(kWeights.data(), 6);
       CHECK(ok == (hostRays && e.points == 6), std::string("set_host_weights(6) from ") + kStateName[e.state]);
       if (ok) {
         e.state = HW;
         e.dirty = true;
       }
     }},
    {"set_host_weights(0)", [](RaySource &s, Expect &e) {
       CHECK(s.set_host_weights(nullptr, 0), std::string("set_host_weights(0) from ") + kStateName[e.state]);
       if (e.state == HW)
         e.state = H;
       e.dirty = true;
     }},
    // the clearing calls: the first two drop any source, the last two only their own
    {"set_grid(0)", [](RaySource &s, Expect &e) {
       s.set_grid(nullptr, 0);
       to_random(e, true);
     }},
    {"set_host_rays(0)", [](RaySource &s, Expect &e) {
       s.set_host_rays(nullptr, nullptr, nullptr, 0);
       to_random(e, true);
     }},
    {"clear_if(Surface)", [](RaySource &s, Expect &e) {
       const bool changed = s.clear_if(SourceKind::Surface);
       CHECK(changed == (e.state == S), std::string("clear_if(Surface) from ") + kStateName[e.state]);
       if (e.state == S)
         to_random(e, e.dirty);
     }},
    {"clear_if(Model)", [](RaySource &s, Expect &e) {
       const bool changed = s.clear_if(SourceKind::Model);
       CHECK(changed == (e.state == M || e.state == MW), std::string("clear_if(Model) from ") + kStateName[e.state]);
       if (e.state == M || e.state == MW)
         to_random(e, e.dirty);
     }},
};

// the five kinds to start from, each with a payload (host rays with weights, a model with kHasWeight and its own count)
static void start(int kind, RaySource &s, Expect &e) {
  s = RaySource{};
  e = Expect{};
  switch (kind) {
  case 0: break;
  case 1:
    s.set_grid(kFloats.data(), 4);
    e = Expect{G, 4};
    e.dirty = true;
    break;
  case 2:
    s.set_host_rays(kFloats.data(), kDirs.data(), kDraws.data(), 6);
    s.set_host_weights(kWeights.data(), 6);
    e = Expect{HW, 6, 0, true};
    e.dirty = true;
    break;
  case 3:
    s.set_surface(2, 1.f, 0.25f);
    e = Expect{S, 2};
    e.area = 1.f;
    e.offset = 0.25f;
    break;
  case 4:
    s.set_model(2, true, kParams, 3, 9, 9);
    e = Expect{MW, 0, 9};
    e.model = 2;
    e.nparams = 3;
    e.table = 9;
    break;
  }
}

int main() {
  int steps = 0;
  for (int kind = 0; kind < 5; ++kind)
    for (const Step &first : kSteps)
      for (const Step &second : kSteps) { // (two steps: every call also from the states only a call can reach)
        RaySource s;
        Expect e;
        start(kind, s, e);
        std::string what = std::string(kStateName[e.state]);
        check(s, e, what);
        first.run(s, e);
        what += std::string(" -> ") + first.name;
        check(s, e, what);
        second.run(s, e);
        what += std::string(" -> ") + second.name;
        check(s, e, what);
        steps += 2;
      }
  if (failures) {
    std::printf("source state: %d checks FAILED\n", failures);
    return 1;
  }
  std::printf("source state ok: %d steps\n", steps);
  return 0;
}
