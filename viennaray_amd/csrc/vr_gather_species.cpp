// vr_gather_species.cpp — vr_gather_species* : up to VR_GATHER_MAX_SPECIES species weighed along one set of traced paths
// (include/viennaray_amd.h has the definition; vr_gather_species.hip the kernel, vr_gather.hpp the per-species step and
// the weight rule).  Species s is one vr_gather_spec plus an optional vr_gather_laws and means what vr_gather_angular means
// by that pair: every check of a species is the angular call's own (paths_refusal, gather_laws_refusal), made under a
// name that carries the species.  One species IS the angular call and goes to its implementation.  Like the other gather
// calls these prepare nothing and touch none of prepared / launched / haveResult; the work buffers are the gather's
// (sums, laws, reflectivities in leaf order, staging), grown to numSpecies of each.
// vr_gather_species_adaptive* are the rounds of vr_gather_adaptive.cpp over those sums, with a mask of species per listed
// primitive: a species that has met its own target stops there and no longer keeps the shared path alive.
#include <algorithm>
#include <cmath>
#include <string>

#include "vr_context.hpp"
#include "vr_gather.hpp"

static_assert(VR_GATHER_MAX_SPECIES == vr::GATHER_MAX_SPECIES && VR_GATHER_MAX_SPECIES == vr::GATHER_SPECIES_MAX,
              "vr_gather.hpp's and vr_kernels.hpp's bounds are the header's");

namespace vr {

constexpr size_t LAW_WORDS = 3 * GATHER_LAW_MAX; // a species' three laws on the device

static std::string species_name(const char *api, uint32_t s) { return std::string(api) + ": species " + std::to_string(s); }

// there are specs to read, and as many as a call takes
static int species_count_refusal(vr_context *c, const char *api, const vr_gather_spec *specs, uint32_t S) {
  const std::string name = api;
  if (!specs)
    return fail(c, VR_E_INVALID, (name + ": specs must not be null").c_str());
  if (S == 0 || S > VR_GATHER_MAX_SPECIES)
    return fail(c, VR_E_INVALID, (name + ": numSpecies must be 1 .. VR_GATHER_MAX_SPECIES (4)").c_str());
  return VR_OK;
}

// what every form refuses before it touches anything; samples: the call's, or the budget; out: a non-null output.
// sets[s]: the laws of species s, normalised
static int species_refusal(vr_context *c, const char *api, const vr_gather_spec *specs, const vr_gather_laws *laws, uint32_t S,
                           uint32_t primFirst, uint32_t primCount, uint32_t samples, const void *out, GatherLawSet *sets) {
  VR_TRY(species_count_refusal(c, api, specs, S));
  for (uint32_t s = 0; s < S; ++s) {
    const vr_gather_spec &sp = specs[s];
    const std::string who = species_name(api, s);
    if (sp.paths != 1u || sp.mode != VR_GATHER_NORMAL || sp.emission)
      return fail(c, VR_E_INVALID, (who + ": spec.paths must be 1, spec.mode VR_GATHER_NORMAL and spec.emission NULL").c_str());
    if (sp.reflection != specs[0].reflection || sp.maxBounces != specs[0].maxBounces)
      return fail(c, VR_E_INVALID, (who + ": reflection and maxBounces are the path's: they must be those of species 0").c_str());
    VR_TRY(paths_refusal(c, who.c_str(), primFirst, primCount, samples, sp.cosinePower, sp.reflection, sp.maxBounces, sp.reflectivity,
                         sp.reflectivityScalar, out));
    VR_TRY(gather_laws_refusal(c, who.c_str(), laws ? &laws[s] : nullptr, sp.cosinePower, samples, sets[s]));
  }
  return VR_OK;
}

// the species' tables (device memory, by original id; nullptr: a scalar) into leaf order, species s at c->dPathRho + s n,
// and their verdicts: one copy back, a word per species — the lowest refused index
static int species_tables(vr_context *c, const char *api, const float *const *rho, uint32_t S, bool &waited) {
  const uint32_t n = c->geo.numPrims;
  bool any = false;
  for (uint32_t s = 0; s < S; ++s)
    any = any || rho[s];
  if (!any)
    return VR_OK;
  VR_TRY(map_grow(c, c->dPathRho, (size_t)S * n, waited));
  VR_TRY(map_grow(c, c->dPathWord, VR_GATHER_MAX_SPECIES, waited));
  VR_HIP(c, hipMemsetAsync(c->dPathWord.p, 0xFF, 4 * VR_GATHER_MAX_SPECIES, c->stream));
  for (uint32_t s = 0; s < S; ++s)
    if (rho[s])
      VR_HIP(c, launch_radiosity_rho(rho[s], 0.f, c->dLeafOfOrig.p, n, c->dPathRho.p + (size_t)s * n, c->dPathWord.p + s, c->stream));
  uint32_t first[VR_GATHER_MAX_SPECIES];
  VR_HIP(c, hipMemcpyAsync(first, c->dPathWord.p, sizeof(first), hipMemcpyDeviceToHost, c->stream));
  VR_TRY(host_waits(c));
  for (uint32_t s = 0; s < S; ++s)
    if (rho[s] && first[s] != 0xFFFFFFFFu)
      return fail(c, VR_E_INVALID, (species_name(api, s) + ": reflectivity[" + std::to_string(first[s]) +
                                    "] is NaN, negative or above 1 (the lowest such index)")
                                       .c_str());
  return VR_OK;
}

// host tables onto the device (c->dPathIn, species s at s n), then species_tables
static int species_upload(vr_context *c, const char *api, const vr_gather_spec *specs, uint32_t S, bool &waited) {
  const uint32_t n = c->geo.numPrims;
  const float *rho[VR_GATHER_MAX_SPECIES] = {nullptr, nullptr, nullptr, nullptr};
  bool any = false;
  for (uint32_t s = 0; s < S; ++s)
    any = any || specs[s].reflectivity;
  if (!any)
    return VR_OK;
  VR_TRY(map_grow(c, c->dPathIn, (size_t)S * n, waited));
  for (uint32_t s = 0; s < S; ++s)
    if (specs[s].reflectivity) {
      rho[s] = c->dPathIn.p + (size_t)s * n;
      VR_HIP(c, hipMemcpyAsync(c->dPathIn.p + (size_t)s * n, specs[s].reflectivity, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    }
  return species_tables(c, api, rho, S, waited);
}

// the launch arguments: what the species share (a path gather's, of `samples` samples) and each one's own; the laws go
// to the device as the angular call's do, a table per species.  A species with a table has passed species_tables
static int species_args(vr_context *c, bool &waited, TraceParams &p, GatherSpeciesArgs &sa, const vr_gather_spec *specs,
                        const GatherLawSet *sets, uint32_t S, uint32_t primFirst, uint32_t primCount, uint32_t samples) {
  sa = GatherSpeciesArgs{};
  VR_TRY(gather_params(c, waited, p, sa.a, primFirst, primCount, samples, 1.f, VR_GATHER_NORMAL));
  if (primCount == c->geo.numPrims)
    sa.a.leafOfOrig = nullptr; // the whole scene: in leaf order
  sa.a.paths = 1u;
  sa.a.reflection = specs[0].reflection;
  sa.a.maxBounces = specs[0].maxBounces;
  sa.num = S;
  const uint32_t n = c->geo.numPrims;
  bool anyLaw = false;
  for (uint32_t s = 0; s < S; ++s) {
    sa.rho[s] = specs[s].reflectivityScalar;
    sa.rhoLeaf[s] = specs[s].reflectivity ? c->dPathRho.p + (size_t)s * n : nullptr;
    sa.cosinePower[s] = specs[s].cosinePower;
    sa.g[s] = gather_g(specs[s].cosinePower, c->geo.D);
    sa.gL[s] = sets[s].gL;
    for (int w = 0; w < 3; ++w)
      sa.lawCount[s][w] = sets[s].count[w];
    anyLaw = anyLaw || sets[s].any;
  }
  if (anyLaw) {
    VR_TRY(map_grow(c, c->dGatherLaws, VR_GATHER_MAX_SPECIES * LAW_WORDS, waited));
    for (uint32_t s = 0; s < S; ++s) // (a species without laws puts its zeros: the kernel stages S whole tables)
      VR_HIP(c, launch_gather_laws(sets[s].table, c->dGatherLaws.p + s * LAW_WORDS, c->stream));
    sa.laws = c->dGatherLaws.p;
  }
  return VR_OK;
}

// the kernels of a fixed-K call, on the context's stream: every pointer is device memory, the arguments have been
// accepted; out: S x primCount floats
static int species_on_device(vr_context *c, const vr_gather_spec *specs, const GatherLawSet *sets, uint32_t S, uint32_t primFirst,
                             uint32_t primCount, uint32_t samples, float *out) {
  bool waited = false;
  VR_TRY(map_grow(c, c->dGatherAcc, (size_t)S * primCount, waited));
  TraceParams p;
  GatherSpeciesArgs sa;
  VR_TRY(species_args(c, waited, p, sa, specs, sets, S, primFirst, primCount, samples));
  sa.a.acc = c->dGatherAcc.p;
  VR_HIP(c, hipMemsetAsync(c->dGatherAcc.p, 0, (size_t)S * primCount * 8, c->stream));
  const unsigned slabs = (unsigned)std::min<size_t>(c->walkStackWaves, 0xFFFFFFFFu);
  gather_cut_chunks(sa.a, slabs);
  VR_HIP(c, launch_gather_species(p, c->geo.geo, c->geo.D, sa, slabs, c->stream));
  for (uint32_t s = 0; s < S; ++s)
    VR_HIP(c, launch_gather_finish(c->dGatherAcc.p + (size_t)s * primCount, primCount, samples, out + (size_t)s * primCount, c->stream));
  return VR_OK;
}

// chunks [chunkFirst, chunkFirst + chunks) of a call of `budget` samples into sum / sumSq (device, S x primCount each)
static int species_sums_on_device(vr_context *c, const vr_gather_spec *specs, const GatherLawSet *sets, uint32_t S, uint32_t primFirst,
                                  uint32_t primCount, uint32_t chunkFirst, uint32_t chunks, uint32_t budget, unsigned long long *sum,
                                  unsigned long long *sumSq) {
  bool waited = false;
  TraceParams p;
  GatherSpeciesArgs sa;
  VR_TRY(species_args(c, waited, p, sa, specs, sets, S, primFirst, primCount, budget));
  VR_HIP(c, hipMemsetAsync(sum, 0, (size_t)S * primCount * 8, c->stream));
  VR_HIP(c, hipMemsetAsync(sumSq, 0, (size_t)S * primCount * 8, c->stream));
  if (chunks == 0)
    return VR_OK;
  GatherArgs &a = sa.a;
  a.stat = 1u;
  a.acc = sum;
  a.accSq = sumSq;
  a.chunkFirst = chunkFirst;
  a.chunks = chunks;
  a.samples = (chunkFirst + chunks) * GATHER_CHUNK; // (<= the budget <= 2^22: the entry points' checks)
  const unsigned slabs = (unsigned)std::min<size_t>(c->walkStackWaves, 0xFFFFFFFFu);
  gather_cut_chunks(a, slabs);
  VR_HIP(c, launch_gather_species(p, c->geo.geo, c->geo.D, sa, slabs, c->stream));
  return VR_OK;
}

static int species_sums_refusal(vr_context *c, const char *api, const vr_gather_spec *specs, const vr_gather_laws *laws, uint32_t S,
                                uint32_t primFirst, uint32_t primCount, uint32_t chunkFirst, uint32_t chunks, uint32_t budget,
                                const void *sum, const void *sumSq, GatherLawSet *sets) {
  VR_TRY(species_refusal(c, api, specs, laws, S, primFirst, primCount, budget, sum && sumSq ? sum : nullptr, sets));
  if (((uint64_t)chunkFirst + chunks) * GATHER_CHUNK > budget)
    return fail(c, VR_E_INVALID, (std::string(api) + ": the chunks end beyond the budget: 64 (chunkFirst + chunks) > budget").c_str());
  return VR_OK;
}

// ---- vr_gather_species_adaptive*: every species of a primitive to its own target, along one set of paths ---------------
// what both forms refuse before they touch anything: vr_gather_adaptive's checks, the targets per species, then what
// vr_gather_species refuses at samples = maxSamples
static int species_adaptive_refusal(vr_context *c, const char *api, const vr_gather_spec *specs, const vr_gather_laws *laws, uint32_t S,
                                    uint32_t primFirst, uint32_t primCount, uint32_t minSamples, uint32_t maxSamples, const float *rel,
                                    const float *abs, const void *flux, const void *info, GatherLawSet *sets) {
  const std::string name = api;
  if (minSamples == 0 || minSamples % GATHER_CHUNK)
    return fail(c, VR_E_INVALID, (name + ": minSamples must be a positive multiple of 64").c_str());
  const uint32_t ratio = maxSamples / minSamples;
  if (maxSamples % minSamples || ratio == 0 || (ratio & (ratio - 1u)))
    return fail(c, VR_E_INVALID, (name + ": maxSamples must be minSamples times a power of two").c_str());
  VR_TRY(species_count_refusal(c, api, specs, S)); // (the targets are numSpecies floats each)
  if (!rel || !abs)
    return fail(c, VR_E_INVALID, (name + ": relTargets and absTargets must not be null (numSpecies floats each)").c_str());
  for (uint32_t s = 0; s < S; ++s)
    if (!(rel[s] >= 0.f) || !(abs[s] >= 0.f))
      return fail(c, VR_E_INVALID, (species_name(api, s) + ": the targets must not be negative or NaN").c_str());
  if (!info)
    return fail(c, VR_E_INVALID, (name + ": info must not be null").c_str());
  return species_refusal(c, api, specs, laws, S, primFirst, primCount, maxSamples, flux, sets);
}

// one species: the angular adaptive call itself, its info in the species call's form
static void species_info_of_one(const vr_gather_adaptive_info &one, vr_gather_species_adaptive_info &info) {
  info = vr_gather_species_adaptive_info{};
  info.rounds = one.rounds;
  info.unconverged[0] = one.unconverged;
  info.totalSamples[0] = one.totalSamples;
  info.walkedSamples = one.totalSamples;
}

// The rounds (vr_gather_adaptive.cpp: adaptive_on_device, for S >= 2 species).  Every pointer is device memory (stdErr,
// samplesUsed: or nullptr), S x primCount each, the arguments have been accepted.  Work buffers: the S x primCount sums and
// sums of squares, two lists with their masks behind them (2 primCount words each), the decide kernel's block counts and
// five words per round.  The host waits once per round, for those five words: the next list's length and, per species,
// the entries it is still sampling in — from which totalSamples and rounds of every species follow without a pass over
// the outputs
static int species_adaptive_on_device(vr_context *c, const vr_gather_spec *specs, const GatherLawSet *sets, uint32_t S, uint32_t primFirst,
                                      uint32_t primCount, uint32_t minSamples, uint32_t maxSamples, const float *rel, const float *abs,
                                      float *flux, float *stdErr, uint32_t *samplesUsed, vr_gather_species_adaptive_info &info) {
  constexpr uint32_t ROUND_WORDS = 1u + VR_GATHER_MAX_SPECIES;
  bool waited = false;
  const uint32_t blocks = (uint32_t)(((uint64_t)primCount + GATHER_DECIDE_BLOCK - 1u) / GATHER_DECIDE_BLOCK);
  uint32_t rounds = 1u;
  for (uint32_t k = minSamples; k < maxSamples; k *= 2u)
    ++rounds;
  VR_TRY(map_grow(c, c->dGatherAcc, (size_t)S * primCount, waited));
  VR_TRY(map_grow(c, c->dGatherAccSq, (size_t)S * primCount, waited));
  VR_TRY(map_grow(c, c->dGatherListA, (size_t)2 * primCount, waited));
  VR_TRY(map_grow(c, c->dGatherListB, (size_t)2 * primCount, waited));
  VR_TRY(map_grow(c, c->dGatherWords, (size_t)blocks + (size_t)rounds * ROUND_WORDS, waited));
  TraceParams p;
  GatherSpeciesArgs sa;
  VR_TRY(species_args(c, waited, p, sa, specs, sets, S, primFirst, primCount, maxSamples));
  GatherArgs &a = sa.a;
  a.stat = 1u;
  a.acc = c->dGatherAcc.p;
  a.accSq = c->dGatherAccSq.p;
  VR_HIP(c, hipMemsetAsync(a.acc, 0, (size_t)S * primCount * 8, c->stream));
  VR_HIP(c, hipMemsetAsync(a.accSq, 0, (size_t)S * primCount * 8, c->stream));
  VR_HIP(c, hipMemsetAsync(c->dGatherWords.p + blocks, 0, (size_t)rounds * ROUND_WORDS * 4, c->stream));
  GatherSpeciesDecideArgs d{};
  d.acc = a.acc;
  d.accSq = a.accSq;
  if (!a.leafOfOrig) { // the whole scene: a list entry is a leaf position, the sums' index the record's original id
    d.origWords = reinterpret_cast<const uint32_t *>(p.prims);
    d.origStride = c->geo.geo == 0 ? 8u : 16u;
    d.origOffset = c->geo.geo == 0 ? 7u : 3u;
  }
  d.blockCounts = c->dGatherWords.p;
  d.flux = flux;
  d.stdErr = stdErr;
  d.samplesUsed = samplesUsed;
  d.primCount = primCount;
  d.num = S;
  for (uint32_t s = 0; s < S; ++s)
    d.rel[s] = rel[s], d.abs[s] = abs[s];
  const unsigned slabs = (unsigned)std::min<size_t>(c->walkStackWaves, 0xFFFFFFFFu);
  const uint32_t c0 = minSamples / GATHER_CHUNK;
  const uint32_t *list = nullptr, *masks = nullptr;
  uint32_t listCount = primCount;
  uint32_t sampling[VR_GATHER_MAX_SPECIES] = {0u, 0u, 0u, 0u}; // entries species s samples in this round
  for (uint32_t s = 0; s < S; ++s)
    sampling[s] = primCount;
  info = vr_gather_species_adaptive_info{};
  for (uint32_t r = 0;; ++r) {
    const uint32_t chunkFirst = r == 0 ? 0u : c0 << (r - 1u), chunks = r == 0 ? c0 : c0 << (r - 1u);
    const uint32_t K = (chunkFirst + chunks) * GATHER_CHUNK; // (<= maxSamples <= 2^22: the entry points' checks)
    a.chunkFirst = chunkFirst;
    a.chunks = chunks;
    a.samples = K;
    a.list = list;
    a.listCount = list ? listCount : 0u;
    sa.listMask = masks;
    a.groups = (uint32_t)(((uint64_t)listCount + 63) / 64);
    a.subs = 1u;
    gather_cut_chunks(a, slabs); // per launch: the late rounds have few primitives
    VR_HIP(c, launch_gather_species(p, c->geo.geo, c->geo.D, sa, slabs, c->stream));
    const uint64_t roundSamples = (uint64_t)chunks * GATHER_CHUNK;
    info.walkedSamples += (uint64_t)listCount * roundSamples;
    for (uint32_t s = 0; s < S; ++s)
      info.totalSamples[s] += (uint64_t)sampling[s] * roundSamples;
    ++info.rounds; // (the list is not empty: one species at least samples in this round)
    uint32_t *const next = (r & 1u) ? c->dGatherListB.p : c->dGatherListA.p;
    d.list = list;
    d.masks = masks;
    d.count = listCount;
    d.samples = K;
    d.last = K == maxSamples ? 1u : 0u;
    d.next = next;
    d.nextMasks = next + primCount;
    d.words = c->dGatherWords.p + blocks + (size_t)r * ROUND_WORDS;
    VR_HIP(c, launch_gather_species_decide(d, c->stream));
    uint32_t words[ROUND_WORDS];
    VR_HIP(c, hipMemcpyAsync(words, d.words, sizeof(words), hipMemcpyDeviceToHost, c->stream));
    VR_TRY(host_waits(c));
    if (d.last) {
      for (uint32_t s = 0; s < S; ++s)
        info.unconverged[s] = words[1u + s];
      break;
    }
    if (words[0] == 0u)
      break;
    list = next;
    masks = next + primCount;
    listCount = words[0];
    for (uint32_t s = 0; s < S; ++s)
      sampling[s] = words[1u + s];
  }
  return VR_OK;
}

} // namespace vr

using namespace vr;

extern "C" {

int vr_gather_species_device(vr_context *c, const vr_gather_spec *specs, const vr_gather_laws *laws, uint32_t S, uint32_t primFirst,
                             uint32_t primCount, uint32_t samples, float *out, void *stream) {
  if (!c)
    return VR_E_INVALID;
  const char *api = "vr_gather_species_device";
  GatherLawSet sets[VR_GATHER_MAX_SPECIES];
  VR_TRY(species_refusal(c, api, specs, laws, S, primFirst, primCount, samples, out, sets));
  if (S == 1u) // (one species: the angular call itself)
    return paths_call_device(c, api, laws, primFirst, primCount, samples, specs->cosinePower, specs->reflection, specs->maxBounces,
                             specs->reflectivity, specs->reflectivityScalar, out, stream);
  VR_TRY(resident_scene_refusal(c, api, "gather from"));
  const float *rho[VR_GATHER_MAX_SPECIES] = {nullptr, nullptr, nullptr, nullptr};
  for (uint32_t s = 0; s < S; ++s)
    rho[s] = specs[s].reflectivity;
  VR_TRY(hand_over(c, {rho[0], rho[1], rho[2], rho[3], out},
                   (std::string(api) + ": the species' reflectivity tables and out must be device memory of the context's device").c_str(),
                   stream));
  bool waited = false;
  VR_TRY(species_tables(c, api, rho, S, waited));
  if (primCount == 0)
    return caller_waits(c, stream);
  VR_TRY(species_on_device(c, specs, sets, S, primFirst, primCount, samples, out));
  return caller_waits(c, stream);
}

int vr_gather_species(vr_context *c, const vr_gather_spec *specs, const vr_gather_laws *laws, uint32_t S, uint32_t primFirst,
                      uint32_t primCount, uint32_t samples, float *out) {
  if (!c)
    return VR_E_INVALID;
  const char *api = "vr_gather_species";
  GatherLawSet sets[VR_GATHER_MAX_SPECIES];
  VR_TRY(species_refusal(c, api, specs, laws, S, primFirst, primCount, samples, out, sets));
  if (S == 1u)
    return paths_call_host(c, api, laws, primFirst, primCount, samples, specs->cosinePower, specs->reflection, specs->maxBounces,
                           specs->reflectivity, specs->reflectivityScalar, out);
  VR_TRY(resident_scene_refusal(c, api, "gather from"));
  VR_HIP(c, hipSetDevice(c->device));
  bool waited = false;
  VR_TRY(species_upload(c, api, specs, S, waited));
  if (primCount == 0)
    return VR_OK;
  VR_TRY(map_grow(c, c->dGatherOut, (size_t)S * primCount, waited));
  VR_TRY(species_on_device(c, specs, sets, S, primFirst, primCount, samples, c->dGatherOut.p));
  VR_HIP(c, hipMemcpyAsync(out, c->dGatherOut.p, (size_t)S * primCount * 4, hipMemcpyDeviceToHost, c->stream));
  VR_HIP(c, hipStreamSynchronize(c->stream));
  return VR_OK;
}

int vr_gather_species_sums_device(vr_context *c, const vr_gather_spec *specs, const vr_gather_laws *laws, uint32_t S,
                                  uint32_t primFirst, uint32_t primCount, uint32_t chunkFirst, uint32_t chunks, uint32_t budget,
                                  int64_t *sum, int64_t *sumSq, void *stream) {
  if (!c)
    return VR_E_INVALID;
  const char *api = "vr_gather_species_sums_device";
  GatherLawSet sets[VR_GATHER_MAX_SPECIES];
  VR_TRY(species_sums_refusal(c, api, specs, laws, S, primFirst, primCount, chunkFirst, chunks, budget, sum, sumSq, sets));
  if (S == 1u)
    return sums_call_device(c, api, specs, laws, primFirst, primCount, chunkFirst, chunks, budget, sum, sumSq, stream);
  VR_TRY(resident_scene_refusal(c, api, "gather from"));
  const float *rho[VR_GATHER_MAX_SPECIES] = {nullptr, nullptr, nullptr, nullptr};
  for (uint32_t s = 0; s < S; ++s)
    rho[s] = specs[s].reflectivity;
  VR_TRY(hand_over(c, {rho[0], rho[1], rho[2], rho[3], sum, sumSq},
                   (std::string(api) + ": the species' reflectivity tables, sum and sumSq must be device memory of the context's device")
                       .c_str(),
                   stream));
  bool waited = false;
  VR_TRY(species_tables(c, api, rho, S, waited));
  if (primCount == 0)
    return caller_waits(c, stream);
  VR_TRY(species_sums_on_device(c, specs, sets, S, primFirst, primCount, chunkFirst, chunks, budget,
                                reinterpret_cast<unsigned long long *>(sum), reinterpret_cast<unsigned long long *>(sumSq)));
  return caller_waits(c, stream);
}

int vr_gather_species_sums(vr_context *c, const vr_gather_spec *specs, const vr_gather_laws *laws, uint32_t S, uint32_t primFirst,
                           uint32_t primCount, uint32_t chunkFirst, uint32_t chunks, uint32_t budget, int64_t *sum, int64_t *sumSq) {
  if (!c)
    return VR_E_INVALID;
  const char *api = "vr_gather_species_sums";
  GatherLawSet sets[VR_GATHER_MAX_SPECIES];
  VR_TRY(species_sums_refusal(c, api, specs, laws, S, primFirst, primCount, chunkFirst, chunks, budget, sum, sumSq, sets));
  if (S == 1u)
    return sums_call_host(c, api, specs, laws, primFirst, primCount, chunkFirst, chunks, budget, sum, sumSq);
  VR_TRY(resident_scene_refusal(c, api, "gather from"));
  VR_HIP(c, hipSetDevice(c->device));
  bool waited = false;
  VR_TRY(species_upload(c, api, specs, S, waited));
  if (primCount == 0)
    return VR_OK;
  VR_TRY(map_grow(c, c->dGatherAcc, (size_t)S * primCount, waited));
  VR_TRY(map_grow(c, c->dGatherAccSq, (size_t)S * primCount, waited));
  VR_TRY(species_sums_on_device(c, specs, sets, S, primFirst, primCount, chunkFirst, chunks, budget, c->dGatherAcc.p, c->dGatherAccSq.p));
  VR_HIP(c, hipMemcpyAsync(sum, c->dGatherAcc.p, (size_t)S * primCount * 8, hipMemcpyDeviceToHost, c->stream));
  VR_HIP(c, hipMemcpyAsync(sumSq, c->dGatherAccSq.p, (size_t)S * primCount * 8, hipMemcpyDeviceToHost, c->stream));
  VR_HIP(c, hipStreamSynchronize(c->stream));
  return VR_OK;
}

int vr_gather_species_adaptive_device(vr_context *c, const vr_gather_spec *specs, const vr_gather_laws *laws, uint32_t S,
                                      uint32_t primFirst, uint32_t primCount, uint32_t minSamples, uint32_t maxSamples,
                                      const float *relTargets, const float *absTargets, float *flux, float *stdErr,
                                      uint32_t *samplesUsed, vr_gather_species_adaptive_info *info, void *stream) {
  if (!c)
    return VR_E_INVALID;
  const char *api = "vr_gather_species_adaptive_device";
  GatherLawSet sets[VR_GATHER_MAX_SPECIES];
  VR_TRY(species_adaptive_refusal(c, api, specs, laws, S, primFirst, primCount, minSamples, maxSamples, relTargets, absTargets, flux, info,
                                  sets));
  if (S == 1u) { // (one species: the angular adaptive call itself)
    vr_gather_adaptive_info one{};
    VR_TRY(adaptive_call_device(c, api, specs, laws, primFirst, primCount, minSamples, maxSamples, relTargets[0], absTargets[0], flux,
                                stdErr, samplesUsed, &one, stream));
    species_info_of_one(one, *info);
    return VR_OK;
  }
  VR_TRY(resident_scene_refusal(c, api, "gather from"));
  const float *rho[VR_GATHER_MAX_SPECIES] = {nullptr, nullptr, nullptr, nullptr};
  for (uint32_t s = 0; s < S; ++s)
    rho[s] = specs[s].reflectivity;
  VR_TRY(hand_over(c, {rho[0], rho[1], rho[2], rho[3], flux, stdErr, samplesUsed},
                   (std::string(api) +
                    ": the species' reflectivity tables, flux, stdErr and samplesUsed must be device memory of the context's device")
                       .c_str(),
                   stream));
  bool waited = false;
  VR_TRY(species_tables(c, api, rho, S, waited));
  *info = vr_gather_species_adaptive_info{};
  if (primCount == 0)
    return caller_waits(c, stream);
  VR_TRY(species_adaptive_on_device(c, specs, sets, S, primFirst, primCount, minSamples, maxSamples, relTargets, absTargets, flux, stdErr,
                                    samplesUsed, *info));
  return caller_waits(c, stream);
}

int vr_gather_species_adaptive(vr_context *c, const vr_gather_spec *specs, const vr_gather_laws *laws, uint32_t S, uint32_t primFirst,
                               uint32_t primCount, uint32_t minSamples, uint32_t maxSamples, const float *relTargets,
                               const float *absTargets, float *flux, float *stdErr, uint32_t *samplesUsed,
                               vr_gather_species_adaptive_info *info) {
  if (!c)
    return VR_E_INVALID;
  const char *api = "vr_gather_species_adaptive";
  GatherLawSet sets[VR_GATHER_MAX_SPECIES];
  VR_TRY(species_adaptive_refusal(c, api, specs, laws, S, primFirst, primCount, minSamples, maxSamples, relTargets, absTargets, flux, info,
                                  sets));
  if (S == 1u) {
    vr_gather_adaptive_info one{};
    VR_TRY(adaptive_call_host(c, api, specs, laws, primFirst, primCount, minSamples, maxSamples, relTargets[0], absTargets[0], flux, stdErr,
                              samplesUsed, &one));
    species_info_of_one(one, *info);
    return VR_OK;
  }
  VR_TRY(resident_scene_refusal(c, api, "gather from"));
  VR_HIP(c, hipSetDevice(c->device));
  bool waited = false;
  VR_TRY(species_upload(c, api, specs, S, waited));
  *info = vr_gather_species_adaptive_info{};
  if (primCount == 0)
    return VR_OK;
  const size_t n = (size_t)S * primCount;
  VR_TRY(map_grow(c, c->dGatherOut, n, waited));
  VR_TRY(map_grow(c, c->dGatherErr, n, waited));
  VR_TRY(map_grow(c, c->dGatherUsed, n, waited));
  VR_TRY(species_adaptive_on_device(c, specs, sets, S, primFirst, primCount, minSamples, maxSamples, relTargets, absTargets,
                                    c->dGatherOut.p, c->dGatherErr.p, c->dGatherUsed.p, *info));
  VR_HIP(c, hipMemcpyAsync(flux, c->dGatherOut.p, n * 4, hipMemcpyDeviceToHost, c->stream));
  if (stdErr)
    VR_HIP(c, hipMemcpyAsync(stdErr, c->dGatherErr.p, n * 4, hipMemcpyDeviceToHost, c->stream));
  if (samplesUsed)
    VR_HIP(c, hipMemcpyAsync(samplesUsed, c->dGatherUsed.p, n * 4, hipMemcpyDeviceToHost, c->stream));
  VR_HIP(c, hipStreamSynchronize(c->stream));
  return VR_OK;
}

} // extern "C"
