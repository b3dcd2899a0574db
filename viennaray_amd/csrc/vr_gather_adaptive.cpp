// vr_gather_adaptive.cpp — vr_gather_sums* / vr_gather_adaptive*: the exact int64 sums of a gather's weights and of their
// squares over a range of chunks, and the gather to a target error built on them (include/viennaray_amd.h has the
// definition; vr_gather.hip the kernels — the gather's own sample loop in its STAT instantiations and the decide-and-
// compact kernel — vr_gather.hpp the arithmetic).  Like vr_gather_flux.cpp the calls prepare nothing and touch none of
// prepared / launched / haveResult; they refuse what the fixed-K call of the spec refuses.
#include <algorithm>
#include <cmath>
#include <string>

#include "vr_context.hpp"
#include "vr_gather.hpp"

namespace vr {

// what every form refuses before it touches anything; samples: the budget or maxSamples; out: a non-null output
static int spec_refusal(vr_context *c, const char *api, const vr_gather_spec *s, const vr_gather_laws *lawsIn, GatherLawSet &laws,
                        const struct vr_gather_energy *energyIn, GatherEnergySet &energy, uint32_t primFirst, uint32_t primCount,
                        uint32_t samples, const void *out) {
  const std::string name = api;
  if (!s)
    return fail(c, VR_E_INVALID, (name + ": spec must not be null").c_str());
  if (lawsIn) { // (an angular entry point: the laws weigh a path)
    if (s->paths != 1u || s->mode != VR_GATHER_NORMAL || s->emission)
      return fail(c, VR_E_INVALID, (name + ": angular laws need spec.paths == 1, VR_GATHER_NORMAL and no emission table").c_str());
    VR_TRY(paths_refusal(c, api, primFirst, primCount, samples, s->cosinePower, s->reflection, s->maxBounces, s->reflectivity,
                         s->reflectivityScalar, out));
    VR_TRY(gather_laws_refusal(c, api, lawsIn, s->cosinePower, samples, laws));
    return gather_energy_refusal(c, api, energyIn, laws.wbound, samples, energy); // (an energy entry point has laws, if empty ones)
  }
  if (s->paths > 1u)
    return fail(c, VR_E_INVALID, (name + ": spec.paths is 0 (vr_gather_flux's sample) or 1 (vr_gather_paths's)").c_str());
  if (s->paths == 0u)
    return gather_refusal(c, api, primFirst, primCount, samples, s->cosinePower, s->mode, s->emission, out);
  if (s->mode != VR_GATHER_NORMAL || s->emission)
    return fail(c, VR_E_INVALID, (name + ": a path sample is VR_GATHER_NORMAL and takes no emission table").c_str());
  return paths_refusal(c, api, primFirst, primCount, samples, s->cosinePower, s->reflection, s->maxBounces, s->reflectivity,
                       s->reflectivityScalar, out);
}

// the arguments every launch of a call shares; emission: device memory or nullptr; table: c->dPathRho holds the
// reflectivities (paths_table).  budget: what wmax follows
static int stat_args(vr_context *c, bool &waited, TraceParams &p, GatherArgs &a, const vr_gather_spec &s, const GatherLawSet &laws,
                     const float *emission, bool table, uint32_t primFirst, uint32_t primCount, uint32_t budget) {
  VR_TRY(gather_params(c, waited, p, a, primFirst, primCount, budget, s.cosinePower, s.paths ? VR_GATHER_NORMAL : s.mode));
  VR_TRY(gather_laws_args(c, waited, laws, a));
  if (primCount == c->geo.numPrims)
    a.leafOfOrig = nullptr; // the whole scene: in leaf order
  if (s.paths) {
    a.paths = 1u;
    a.reflection = s.reflection;
    a.maxBounces = s.maxBounces;
    a.rho = s.reflectivityScalar;
    a.rhoLeaf = table ? c->dPathRho.p : nullptr;
  } else {
    a.emission = emission;
  }
  a.stat = 1u;
  return VR_OK;
}

// chunks [chunkFirst, chunkFirst + chunks) of the listed primitives (list == nullptr: of the whole range) into a.acc / a.accSq
static int stat_launch(vr_context *c, const TraceParams &p, GatherArgs a, const GatherEnergyArgs *ea, uint32_t chunkFirst,
                       uint32_t chunks, const uint32_t *list, uint32_t listCount) {
  a.chunkFirst = chunkFirst;
  a.chunks = chunks;
  a.samples = (chunkFirst + chunks) * GATHER_CHUNK; // (<= the budget <= 2^22: the entry points' checks)
  a.list = list;
  a.listCount = listCount;
  a.groups = (uint32_t)(((uint64_t)(list ? listCount : a.primCount) + 63) / 64);
  a.subs = 1u;
  const unsigned slabs = (unsigned)std::min<size_t>(c->walkStackWaves, 0xFFFFFFFFu);
  gather_cut_chunks(a, slabs); // per launch: the late rounds of an adaptive call have few primitives
  return gather_launch(c, p, a, ea, slabs);
}

static int sums_refusal(vr_context *c, const char *api, const vr_gather_spec *s, const vr_gather_laws *lawsIn, GatherLawSet &laws,
                        const struct vr_gather_energy *energyIn, GatherEnergySet &energy, uint32_t primFirst, uint32_t primCount, uint32_t chunkFirst, uint32_t chunks, uint32_t budget,
                        const void *sum, const void *sumSq) {
  VR_TRY(spec_refusal(c, api, s, lawsIn, laws, energyIn, energy, primFirst, primCount, budget, sum && sumSq ? sum : nullptr));
  if (((uint64_t)chunkFirst + chunks) * GATHER_CHUNK > budget)
    return fail(c, VR_E_INVALID, (std::string(api) + ": the chunks end beyond the budget: 64 (chunkFirst + chunks) > budget").c_str());
  return VR_OK;
}

// every pointer is device memory, the arguments have been accepted
static int sums_on_device(vr_context *c, const vr_gather_spec &s, const GatherLawSet &laws, const GatherEnergySet &energy,
                          const float *emission, bool table, uint32_t primFirst,
                          uint32_t primCount, uint32_t chunkFirst, uint32_t chunks, uint32_t budget, unsigned long long *sum,
                          unsigned long long *sumSq) {
  bool waited = false;
  TraceParams p;
  GatherArgs a;
  VR_TRY(stat_args(c, waited, p, a, s, laws, emission, table, primFirst, primCount, budget));
  GatherEnergyArgs ea;
  VR_TRY(gather_energy_args(c, waited, energy, ea));
  VR_HIP(c, hipMemsetAsync(sum, 0, (size_t)primCount * 8, c->stream));
  VR_HIP(c, hipMemsetAsync(sumSq, 0, (size_t)primCount * 8, c->stream));
  if (chunks == 0)
    return VR_OK;
  a.acc = sum;
  a.accSq = sumSq;
  return stat_launch(c, p, a, energy.any ? &ea : nullptr, chunkFirst, chunks, nullptr, 0u);
}

static int adaptive_refusal(vr_context *c, const char *api, const vr_gather_spec *s, const vr_gather_laws *lawsIn,
                            GatherLawSet &laws, const struct vr_gather_energy *energyIn, GatherEnergySet &energy, uint32_t primFirst,
                            uint32_t primCount, uint32_t minSamples, uint32_t maxSamples, float rel, float abs, const void *flux,
                            const void *info) {
  const std::string name = api;
  if (minSamples == 0 || minSamples % GATHER_CHUNK)
    return fail(c, VR_E_INVALID, (name + ": minSamples must be a positive multiple of 64").c_str());
  const uint32_t ratio = maxSamples / minSamples;
  if (maxSamples % minSamples || ratio == 0 || (ratio & (ratio - 1u)))
    return fail(c, VR_E_INVALID, (name + ": maxSamples must be minSamples times a power of two").c_str());
  if (!(rel >= 0.f) || !(abs >= 0.f))
    return fail(c, VR_E_INVALID, (name + ": the targets must not be negative or NaN").c_str());
  if (!info)
    return fail(c, VR_E_INVALID, (name + ": info must not be null").c_str());
  return spec_refusal(c, api, s, lawsIn, laws, energyIn, energy, primFirst, primCount, maxSamples, flux);
}

// The rounds.  Every pointer is device memory (stdErr, samplesUsed: or nullptr), the arguments have been accepted.  The
// host waits once per round for one word, the next list's length
static int adaptive_on_device(vr_context *c, const vr_gather_spec &s, const GatherLawSet &laws, const GatherEnergySet &energy,
                              const float *emission, bool table, uint32_t primFirst,
                              uint32_t primCount, uint32_t minSamples, uint32_t maxSamples, float rel, float abs, float *flux,
                              float *stdErr, uint32_t *samplesUsed, vr_gather_adaptive_info &info) {
  bool waited = false;
  const uint32_t blocks = (uint32_t)(((uint64_t)primCount + GATHER_DECIDE_BLOCK - 1u) / GATHER_DECIDE_BLOCK);
  VR_TRY(map_grow(c, c->dGatherAcc, primCount, waited));
  VR_TRY(map_grow(c, c->dGatherAccSq, primCount, waited));
  VR_TRY(map_grow(c, c->dGatherListA, primCount, waited));
  VR_TRY(map_grow(c, c->dGatherListB, primCount, waited));
  VR_TRY(map_grow(c, c->dGatherWords, (size_t)blocks + 1u, waited));
  TraceParams p;
  GatherArgs a;
  VR_TRY(stat_args(c, waited, p, a, s, laws, emission, table, primFirst, primCount, maxSamples));
  GatherEnergyArgs ea;
  VR_TRY(gather_energy_args(c, waited, energy, ea));
  a.acc = c->dGatherAcc.p;
  a.accSq = c->dGatherAccSq.p;
  VR_HIP(c, hipMemsetAsync(a.acc, 0, (size_t)primCount * 8, c->stream));
  VR_HIP(c, hipMemsetAsync(a.accSq, 0, (size_t)primCount * 8, c->stream));
  GatherDecideArgs d{};
  d.acc = a.acc;
  d.accSq = a.accSq;
  if (!a.leafOfOrig) { // the whole scene: a list entry is a leaf position, the sums' index the record's original id
    d.origWords = reinterpret_cast<const uint32_t *>(p.prims);
    d.origStride = c->geo.geo == 0 ? 8u : 16u;
    d.origOffset = c->geo.geo == 0 ? 7u : 3u;
  }
  d.blockCounts = c->dGatherWords.p;
  d.word = c->dGatherWords.p + blocks;
  d.flux = flux;
  d.stdErr = stdErr;
  d.samplesUsed = samplesUsed;
  d.rel = rel;
  d.abs = abs;
  const uint32_t c0 = minSamples / GATHER_CHUNK;
  const uint32_t *list = nullptr;
  uint32_t listCount = primCount;
  info = vr_gather_adaptive_info{};
  for (uint32_t r = 0;; ++r) {
    const uint32_t chunkFirst = r == 0 ? 0u : c0 << (r - 1u), chunks = r == 0 ? c0 : c0 << (r - 1u);
    const uint32_t K = (chunkFirst + chunks) * GATHER_CHUNK;
    VR_TRY(stat_launch(c, p, a, energy.any ? &ea : nullptr, chunkFirst, chunks, list, listCount));
    info.totalSamples += (uint64_t)listCount * chunks * GATHER_CHUNK;
    ++info.rounds;
    d.list = list;
    d.count = listCount;
    d.samples = K;
    d.last = K == maxSamples ? 1u : 0u;
    d.next = (r & 1u) ? c->dGatherListB.p : c->dGatherListA.p;
    VR_HIP(c, launch_gather_decide(d, c->stream));
    uint32_t kept = 0;
    VR_HIP(c, hipMemcpyAsync(&kept, d.word, 4, hipMemcpyDeviceToHost, c->stream));
    VR_TRY(host_waits(c));
    if (d.last) {
      info.unconverged = kept;
      break;
    }
    if (kept == 0)
      break;
    list = d.next;
    listCount = kept;
  }
  return VR_OK;
}

// a host spec's tables onto the device: emission into c->dGatherEmission, the reflectivities through paths_table
static int spec_upload(vr_context *c, const char *api, const vr_gather_spec &s, bool &waited, const float *&emission, bool &table) {
  const uint32_t n = c->geo.numPrims;
  emission = nullptr;
  table = false;
  if (!s.paths && s.emission) {
    VR_TRY(map_grow(c, c->dGatherEmission, n, waited));
    VR_HIP(c, hipMemcpyAsync(c->dGatherEmission.p, s.emission, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    emission = c->dGatherEmission.p;
  }
  if (s.paths && s.reflectivity) {
    VR_TRY(map_grow(c, c->dPathIn, n, waited));
    VR_HIP(c, hipMemcpyAsync(c->dPathIn.p, s.reflectivity, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    VR_TRY(paths_table(c, api, c->dPathIn.p));
    table = true;
  }
  return VR_OK;
}


int sums_call_device(vr_context *c, const char *api, const vr_gather_spec *spec, const vr_gather_laws *lawsIn, uint32_t primFirst,
                     uint32_t primCount, uint32_t chunkFirst, uint32_t chunks, uint32_t budget, int64_t *sum, int64_t *sumSq,
                     void *stream, const struct vr_gather_energy *energyIn) {
  GatherLawSet laws;
  GatherEnergySet energy;
  VR_TRY(sums_refusal(c, api, spec, lawsIn, laws, energyIn, energy, primFirst, primCount, chunkFirst, chunks, budget, sum, sumSq));
  VR_TRY(resident_scene_refusal(c, api, "gather from"));
  VR_TRY(hand_over(c, {spec->emission, spec->reflectivity, sum, sumSq},
                   (std::string(api) + ": the spec's tables, sum and sumSq must be device memory of the context's device").c_str(),
                   stream));
  const bool table = spec->paths && spec->reflectivity;
  if (table)
    VR_TRY(paths_table(c, api, spec->reflectivity));
  if (primCount == 0)
    return caller_waits(c, stream);
  VR_TRY(sums_on_device(c, *spec, laws, energy, spec->paths ? nullptr : spec->emission, table, primFirst, primCount, chunkFirst, chunks, budget,
                        reinterpret_cast<unsigned long long *>(sum), reinterpret_cast<unsigned long long *>(sumSq)));
  return caller_waits(c, stream);
}

int sums_call_host(vr_context *c, const char *api, const vr_gather_spec *spec, const vr_gather_laws *lawsIn, uint32_t primFirst,
                   uint32_t primCount, uint32_t chunkFirst, uint32_t chunks, uint32_t budget, int64_t *sum, int64_t *sumSq,
                   const struct vr_gather_energy *energyIn) {
  GatherLawSet laws;
  GatherEnergySet energy;
  VR_TRY(sums_refusal(c, api, spec, lawsIn, laws, energyIn, energy, primFirst, primCount, chunkFirst, chunks, budget, sum, sumSq));
  VR_TRY(resident_scene_refusal(c, api, "gather from"));
  VR_HIP(c, hipSetDevice(c->device));
  bool waited = false;
  const float *emission;
  bool table;
  VR_TRY(spec_upload(c, api, *spec, waited, emission, table));
  if (primCount == 0)
    return VR_OK;
  VR_TRY(map_grow(c, c->dGatherAcc, primCount, waited));
  VR_TRY(map_grow(c, c->dGatherAccSq, primCount, waited));
  VR_TRY(sums_on_device(c, *spec, laws, energy, emission, table, primFirst, primCount, chunkFirst, chunks, budget, c->dGatherAcc.p,
                        c->dGatherAccSq.p));
  VR_HIP(c, hipMemcpyAsync(sum, c->dGatherAcc.p, (size_t)primCount * 8, hipMemcpyDeviceToHost, c->stream));
  VR_HIP(c, hipMemcpyAsync(sumSq, c->dGatherAccSq.p, (size_t)primCount * 8, hipMemcpyDeviceToHost, c->stream));
  VR_HIP(c, hipStreamSynchronize(c->stream));
  return VR_OK;
}

int adaptive_call_device(vr_context *c, const char *api, const vr_gather_spec *spec, const vr_gather_laws *lawsIn, uint32_t primFirst,
                         uint32_t primCount, uint32_t minSamples, uint32_t maxSamples, float relTarget, float absTarget,
                         float *flux, float *stdErr, uint32_t *samplesUsed, vr_gather_adaptive_info *info, void *stream,
                         const struct vr_gather_energy *energyIn) {
  GatherLawSet laws;
  GatherEnergySet energy;
  VR_TRY(adaptive_refusal(c, api, spec, lawsIn, laws, energyIn, energy, primFirst, primCount, minSamples, maxSamples, relTarget, absTarget, flux, info));
  VR_TRY(resident_scene_refusal(c, api, "gather from"));
  VR_TRY(hand_over(c, {spec->emission, spec->reflectivity, flux, stdErr, samplesUsed},
                   (std::string(api) + ": the spec's tables, flux, stdErr and samplesUsed must be device memory of the context's device")
                       .c_str(),
                   stream));
  const bool table = spec->paths && spec->reflectivity;
  if (table)
    VR_TRY(paths_table(c, api, spec->reflectivity));
  *info = vr_gather_adaptive_info{};
  if (primCount == 0)
    return caller_waits(c, stream);
  VR_TRY(adaptive_on_device(c, *spec, laws, energy, spec->paths ? nullptr : spec->emission, table, primFirst, primCount, minSamples, maxSamples,
                            relTarget, absTarget, flux, stdErr, samplesUsed, *info));
  return caller_waits(c, stream);
}

int adaptive_call_host(vr_context *c, const char *api, const vr_gather_spec *spec, const vr_gather_laws *lawsIn, uint32_t primFirst,
                       uint32_t primCount, uint32_t minSamples, uint32_t maxSamples, float relTarget, float absTarget, float *flux,
                       float *stdErr, uint32_t *samplesUsed, vr_gather_adaptive_info *info, const struct vr_gather_energy *energyIn) {
  GatherLawSet laws;
  GatherEnergySet energy;
  VR_TRY(adaptive_refusal(c, api, spec, lawsIn, laws, energyIn, energy, primFirst, primCount, minSamples, maxSamples, relTarget, absTarget, flux, info));
  VR_TRY(resident_scene_refusal(c, api, "gather from"));
  VR_HIP(c, hipSetDevice(c->device));
  bool waited = false;
  const float *emission;
  bool table;
  VR_TRY(spec_upload(c, api, *spec, waited, emission, table));
  *info = vr_gather_adaptive_info{};
  if (primCount == 0)
    return VR_OK;
  VR_TRY(map_grow(c, c->dGatherOut, primCount, waited));
  VR_TRY(map_grow(c, c->dGatherErr, primCount, waited));
  VR_TRY(map_grow(c, c->dGatherUsed, primCount, waited));
  VR_TRY(adaptive_on_device(c, *spec, laws, energy, emission, table, primFirst, primCount, minSamples, maxSamples, relTarget, absTarget,
                            c->dGatherOut.p, c->dGatherErr.p, c->dGatherUsed.p, *info));
  VR_HIP(c, hipMemcpyAsync(flux, c->dGatherOut.p, (size_t)primCount * 4, hipMemcpyDeviceToHost, c->stream));
  if (stdErr)
    VR_HIP(c, hipMemcpyAsync(stdErr, c->dGatherErr.p, (size_t)primCount * 4, hipMemcpyDeviceToHost, c->stream));
  if (samplesUsed)
    VR_HIP(c, hipMemcpyAsync(samplesUsed, c->dGatherUsed.p, (size_t)primCount * 4, hipMemcpyDeviceToHost, c->stream));
  VR_HIP(c, hipStreamSynchronize(c->stream));
  return VR_OK;
}

} // namespace vr

using namespace vr;

extern "C" {

int vr_gather_sums_device(vr_context *c, const vr_gather_spec *spec, uint32_t primFirst, uint32_t primCount, uint32_t chunkFirst,
                          uint32_t chunks, uint32_t budget, int64_t *sum, int64_t *sumSq, void *stream) {
  if (!c)
    return VR_E_INVALID;
  return sums_call_device(c, "vr_gather_sums_device", spec, nullptr, primFirst, primCount, chunkFirst, chunks, budget, sum, sumSq,
                          stream);
}

int vr_gather_sums(vr_context *c, const vr_gather_spec *spec, uint32_t primFirst, uint32_t primCount, uint32_t chunkFirst,
                   uint32_t chunks, uint32_t budget, int64_t *sum, int64_t *sumSq) {
  if (!c)
    return VR_E_INVALID;
  return sums_call_host(c, "vr_gather_sums", spec, nullptr, primFirst, primCount, chunkFirst, chunks, budget, sum, sumSq);
}

int vr_gather_adaptive_device(vr_context *c, const vr_gather_spec *spec, uint32_t primFirst, uint32_t primCount,
                              uint32_t minSamples, uint32_t maxSamples, float relTarget, float absTarget, float *flux, float *stdErr,
                              uint32_t *samplesUsed, vr_gather_adaptive_info *info, void *stream) {
  if (!c)
    return VR_E_INVALID;
  return adaptive_call_device(c, "vr_gather_adaptive_device", spec, nullptr, primFirst, primCount, minSamples, maxSamples, relTarget,
                              absTarget, flux, stdErr, samplesUsed, info, stream);
}

int vr_gather_adaptive(vr_context *c, const vr_gather_spec *spec, uint32_t primFirst, uint32_t primCount, uint32_t minSamples,
                       uint32_t maxSamples, float relTarget, float absTarget, float *flux, float *stdErr, uint32_t *samplesUsed,
                       vr_gather_adaptive_info *info) {
  if (!c)
    return VR_E_INVALID;
  return adaptive_call_host(c, "vr_gather_adaptive", spec, nullptr, primFirst, primCount, minSamples, maxSamples, relTarget,
                            absTarget, flux, stdErr, samplesUsed, info);
}

} // extern "C"
