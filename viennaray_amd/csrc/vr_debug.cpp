// vr_debug.cpp — the vr_debug_* entry points: single device functions run on hand-made inputs for the tests, the BVH
// check and the issue-rate microbenchmarks.
#include <algorithm>
#include <cstring>
#include <vector>

#include "vr_context.hpp"

// the debug entry points read the prepared launch: prepare now unless an apply is prepared already
static int ensure_prepared(vr_context *c) { return c->prepared ? VR_OK : vr_apply_prepare(c); }

extern "C" {

// ---- diagnostics ------------------------------------------------------------------
int vr_debug_intersect(vr_context *c, const float *org, const float *dir, const float *tnear, uint32_t n,
                       int32_t *geomID, uint32_t *primID, float *t) {
  if (!c || !org || !dir || !tnear || !geomID || !primID || !t)
    return VR_E_INVALID;
  VR_TRY(ensure_prepared(c));
  DevBuf<float> dO, dD, dT, dt;
  DevBuf<int> dG;
  DevBuf<uint32_t> dP;
  VR_HIP(c, dO.upload(org, (size_t)n * 3));
  VR_HIP(c, dD.upload(dir, (size_t)n * 3));
  VR_HIP(c, dT.upload(tnear, n));
  VR_HIP(c, dt.ensure(n));
  VR_HIP(c, dG.ensure(n));
  VR_HIP(c, dP.ensure(n));
  // the ordered (pair-node, stack) walk of the trace kernels; VR_DEBUG_WALK=0: the escape-link walk it replaced
  const int ordered = read_knobs().debugWalk ? 1 : 0;
  const TraceParams p = launch_params(c, current_launch(c));
  // (64-thread blocks running concurrently must not share a slab: at most walkStackWaves blocks per launch)
  const uint32_t chunk = (uint32_t)std::max<size_t>(c->walkStackWaves, 1) * 64u;
  for (uint32_t f0 = 0; f0 < n; f0 += chunk) {
    const uint32_t m = std::min(chunk, n - f0);
    VR_HIP(c, launch_debug_intersect(p, c->geo.geo, dO.p + 3 * (size_t)f0, dD.p + 3 * (size_t)f0, dT.p + f0, m,
                                     dG.p + f0, dP.p + f0, dt.p + f0, ordered, (unsigned)std::max<size_t>(c->walkStackWaves, 1), c->stream));
  }
  VR_HIP(c, hipStreamSynchronize(c->stream));
  VR_HIP(c, dG.download(geomID, n));
  VR_HIP(c, dP.download(primID, n));
  VR_HIP(c, dt.download(t, n));
  return VR_OK;
}

// Boundary::processHit on the device for hand-built hits (tests/boundaryHit, boundaryHit2D): ray (org, dir) meets wall
// triangle primID at parameter tfar -> new origin, new (projected) direction, reflect flag
int vr_debug_process_hit(vr_context *c, const float *org, const float *dir, const float *tfar, const uint32_t *primID,
                         uint32_t n, float *outOrg, float *outDir, int32_t *outReflect) {
  if (!c || !org || !dir || !tfar || !primID || !outOrg || !outDir || !outReflect)
    return VR_E_INVALID;
  for (uint32_t i = 0; i < n; ++i)
    if (primID[i] > 7u)
      return fail(c, VR_E_INVALID, "vr_debug_process_hit: boundary primID must be 0..7");
  VR_TRY(ensure_prepared(c));
  DevBuf<float> dO, dD, dT, dOo, dDo;
  DevBuf<uint32_t> dP;
  DevBuf<int> dR;
  VR_HIP(c, dO.upload(org, (size_t)n * 3));
  VR_HIP(c, dD.upload(dir, (size_t)n * 3));
  VR_HIP(c, dT.upload(tfar, n));
  VR_HIP(c, dP.upload(primID, n));
  VR_HIP(c, dOo.ensure((size_t)n * 3));
  VR_HIP(c, dDo.ensure((size_t)n * 3));
  VR_HIP(c, dR.ensure(n));
  VR_HIP(c, launch_debug_process_hit(launch_params(c, current_launch(c)), c->geo.D, dO.p, dD.p, dT.p, dP.p, n, dOo.p, dDo.p, dR.p, c->stream));
  VR_HIP(c, hipStreamSynchronize(c->stream));
  VR_HIP(c, dOo.download(outOrg, (size_t)n * 3));
  VR_HIP(c, dDo.download(outDir, (size_t)n * 3));
  VR_HIP(c, dR.download(outReflect, n));
  return VR_OK;
}

int vr_debug_source_sample(vr_context *c, const uint64_t *idx, uint32_t n, uint32_t seed, float *org, float *dir) {
  if (!c || !idx || !org || !dir)
    return VR_E_INVALID;
  if (c->src.kind == SourceKind::Model)
    return fail(c, VR_E_STATE, "vr_debug_source_sample: a source model is set: its sample is vr_debug_user_source_sample's");
  VR_TRY(ensure_prepared(c));
  if (n > c->slotStride)
    return fail(c, VR_E_INVALID, "vr_debug_source_sample: more rays than one batch holds");
  if (c->src.kind == SourceKind::Surface) // (the surface generator looks its point up by the index)
    for (uint32_t i = 0; i < n; ++i)
      if (idx[i] >= rays_of_apply(c))
        return fail(c, VR_E_INVALID, "vr_debug_source_sample: ray index beyond the surface source's ray count");
  const ParticleLaunch &L = current_launch(c);
  TraceParams p = launch_params(c, L);
  p.seed = seed;
  p.batchCount = n;
  p.binCount = nullptr; // no binning: record i goes to slot i
  DevBuf<unsigned long long> dI;
  VR_HIP(c, dI.upload((const unsigned long long *)idx, n));
  p.idxList = dI.p;
  VR_HIP(c, launch_gen(p, L.gen, c->geo.D, false, (unsigned)c->numCUs * 8u, c->stream));
  VR_HIP(c, hipStreamSynchronize(c->stream));
  std::vector<float> A((size_t)n * 8);
  VR_HIP(c, c->dSlotRec.download(A.data(), (size_t)n * 8));
  for (uint32_t i = 0; i < n; ++i) {
    const float *r = &A[8 * (size_t)i];
    org[3 * i] = r[0];
    org[3 * i + 1] = r[1];
    org[3 * i + 2] = r[2];
    dir[3 * i] = r[3];
    dir[3 * i + 1] = r[4];
    dir[3 * i + 2] = r[5];
  }
  return VR_OK;
}

// The surface source's sample (vr_generate.hpp: surface_sample, the device function of its generator) for the global ray
// indices idx[]: origin, direction, start weight and the engine outputs consumed (2)
int vr_debug_surface_source_sample(vr_context *c, const uint64_t *idx, uint32_t n, uint32_t seed, float *org, float *dir,
                                   float *weight, uint32_t *draws) {
  if (!c || !idx || !org || !dir || !weight || !draws)
    return VR_E_INVALID;
  if (c->src.kind != SourceKind::Surface)
    return fail(c, VR_E_STATE, "vr_debug_surface_source_sample: no surface source is set");
  VR_TRY(ensure_prepared(c));
  const uint64_t total = rays_of_apply(c);
  for (uint32_t i = 0; i < n; ++i)
    if (idx[i] >= total)
      return fail(c, VR_E_INVALID, "vr_debug_surface_source_sample: ray index beyond the apply's ray count");
  if (n == 0)
    return VR_OK;
  TraceParams p = launch_params(c, current_launch(c));
  p.seed = seed;
  p.batchCount = n;
  DevBuf<unsigned long long> dI;
  DevBuf<float> dO, dD, dW;
  DevBuf<uint32_t> dK;
  VR_HIP(c, dI.upload((const unsigned long long *)idx, n));
  VR_HIP(c, dO.ensure((size_t)n * 3));
  VR_HIP(c, dD.ensure((size_t)n * 3));
  VR_HIP(c, dW.ensure(n));
  VR_HIP(c, dK.ensure(n));
  p.idxList = dI.p;
  VR_HIP(c, launch_debug_surface_sample(p, (unsigned)c->numCUs * 8u, dO.p, dD.p, dW.p, dK.p, c->stream));
  VR_HIP(c, hipStreamSynchronize(c->stream));
  VR_HIP(c, dO.download(org, (size_t)n * 3));
  VR_HIP(c, dD.download(dir, (size_t)n * 3));
  VR_HIP(c, dW.download(weight, n));
  VR_HIP(c, dK.download(draws, n));
  return VR_OK;
}

// The sample of the source model in force (vr_set_source_model), by the device function its generator calls, for the global
// ray indices idx[] and kernel seed `seed`: origin, direction, start weight (1 without kHasWeight) and the engine outputs
// consumed.  Any index: the sample depends on nothing else.
int vr_debug_user_source_sample(vr_context *c, const uint64_t *idx, uint32_t n, uint32_t seed, float *org, float *dir,
                                float *weight, uint32_t *draws) {
  if (!c || !idx || !org || !dir || !weight || !draws)
    return VR_E_INVALID;
  if (c->src.kind != SourceKind::Model)
    return fail(c, VR_E_STATE, "vr_debug_user_source_sample: no source model is set");
  VR_TRY(ensure_prepared(c));
  if (n == 0)
    return VR_OK;
  const ParticleLaunch &L = current_launch(c);
  TraceParams p = launch_params(c, L);
  SourceCtx sc = L.source;
  p.seed = seed;
  p.batchCount = n;
  DevBuf<unsigned long long> dI;
  DevBuf<float> dO, dD, dW;
  DevBuf<uint32_t> dK;
  VR_HIP(c, dI.upload((const unsigned long long *)idx, n));
  VR_HIP(c, dO.ensure((size_t)n * 3));
  VR_HIP(c, dD.ensure((size_t)n * 3));
  VR_HIP(c, dW.ensure(n));
  VR_HIP(c, dK.ensure(n));
  p.idxList = dI.p;
  void *args[] = {&p, &sc, &dO.p, &dD.p, &dW.p, &dK.p};
  // (the grid bound of the generators: the RNG slabs are sized for it, size_scratch)
  const unsigned grid = std::min<unsigned>((n + VR_BLOCK - 1) / VR_BLOCK, (unsigned)c->numCUs * 8u);
  VR_HIP(c, hipModuleLaunchKernel(c->sourceModels[c->src.sourceModel].debug[c->geo.D == 3 ? 1 : 0], grid, 1, 1, VR_BLOCK, 1, 1, 0,
                                  c->stream, args, nullptr));
  VR_HIP(c, hipStreamSynchronize(c->stream));
  VR_HIP(c, dO.download(org, (size_t)n * 3));
  VR_HIP(c, dD.download(dir, (size_t)n * 3));
  VR_HIP(c, dW.download(weight, n));
  VR_HIP(c, dK.download(draws, n));
  return VR_OK;
}

// vr_debug_source_sample for the active STATEFUL model: its generator (init, then the source sample) for the global ray
// indices idx[]; the first origin, direction and the engine outputs consumed before the trace (init + source)
int vr_debug_model_source_sample(vr_context *c, const uint64_t *idx, uint32_t n, uint32_t seed, float *org, float *dir,
                                 uint32_t *draws) {
  if (!c || !idx || !org || !dir || !draws)
    return VR_E_INVALID;
  VR_TRY(ensure_prepared(c));
  const ParticleLaunch &L = current_launch(c);
  if (c->specs.size() > 1 || !L.userGen || L.gen == GEN_SOURCE_MODEL)
    return fail(c, VR_E_STATE, "vr_debug_model_source_sample: the active particle is not (the only) stateful model");
  if (n > c->batchCap)
    return fail(c, VR_E_INVALID, "vr_debug_model_source_sample: more rays than one batch holds");
  TraceParams p = launch_params(c, L);
  p.seed = seed;
  p.batchCount = n;
  p.binCount = nullptr; // no binning: record i goes to slot i
  DevBuf<unsigned long long> dI;
  VR_HIP(c, dI.upload((const unsigned long long *)idx, n));
  p.idxList = dI.p;
  if (n) {
    void *args[] = {&p};
    const unsigned grid = std::min<unsigned>((n + VR_BLOCK - 1) / VR_BLOCK, (unsigned)c->numCUs * 8u);
    VR_HIP(c, hipModuleLaunchKernel(L.userGen, grid, 1, 1, VR_BLOCK, 1, 1, 0, c->stream, args, nullptr));
  }
  VR_HIP(c, hipStreamSynchronize(c->stream));
  std::vector<float> A((size_t)n * 8), E((size_t)n * 4);
  VR_HIP(c, c->dSlotRec.download(A.data(), (size_t)n * 8));
  VR_HIP(c, c->dRecExtra.download(E.data(), (size_t)n * 4));
  // the compact record {org[firstDir], org[secondDir], dir.x, dir.y} {dir.z, ...} + the side array {org[rayDir], k, ...}
  const int rd = p.rayDir, fd = p.firstDir;
  for (uint32_t i = 0; i < n; ++i) {
    const float *a = &A[8 * (size_t)i], *e = &E[4 * (size_t)i];
    for (int k = 0; k < 3; ++k)
      org[3 * i + k] = k == rd ? e[0] : (k == fd ? a[0] : a[1]);
    dir[3 * i] = a[2];
    dir[3 * i + 1] = a[3];
    dir[3 * i + 2] = a[4];
    std::memcpy(&draws[i], &e[1], 4);
  }
  return VR_OK;
}

int vr_debug_rng_outputs(vr_context *c, uint64_t idx, uint32_t seed, uint32_t count, uint64_t *out) {
  if (!c || !out)
    return VR_E_INVALID;
  VR_HIP(c, hipSetDevice(c->device));
  // tea<3>(idx, seed) on the host (same mix as tea3, vr_rng.hpp)
  unsigned v0 = (unsigned)idx, v1 = seed, s0 = 0;
  for (int n = 0; n < 3; ++n) {
    s0 += 0x9e3779b9u;
    v0 += ((v1 << 4) + 0xa341316cu) ^ (v1 + s0) ^ ((v1 >> 5) + 0xc8013ea4u);
    v1 += ((v0 << 4) + 0xad90777du) ^ (v0 + s0) ^ ((v0 >> 5) + 0x7e95761eu);
  }
  DevBuf<unsigned long long> dS, dOut;
  VR_HIP(c, dS.ensure(312u * 64u));
  VR_HIP(c, dOut.ensure(count));
  VR_HIP(c, launch_debug_rng(v0, count, dS.p, dOut.p, c->stream));
  VR_HIP(c, hipStreamSynchronize(c->stream));
  VR_HIP(c, dOut.download((unsigned long long *)out, count));
  return VR_OK;
}

int vr_debug_bvh_check(vr_context *c, uint32_t *violations) {
  if (!c || !violations)
    return VR_E_INVALID;
  if (!c->haveSetup || c->geometryDirty)
    return fail(c, VR_E_STATE, "vr_debug_bvh_check: no device-built BVH resident (call vr_apply_prepare)");
  VR_HIP(c, hipSetDevice(c->device));
  DevBuf<uint32_t> dBad;
  VR_HIP(c, dBad.ensure(1));
  VR_HIP(c, hipMemsetAsync(dBad.p, 0, 4, c->stream));
  VR_HIP(c, launch_bvh_check(c->lastSetup, dBad.p, c->stream));
  VR_HIP(c, hipMemcpyAsync(violations, dBad.p, 4, hipMemcpyDeviceToHost, c->stream));
  VR_HIP(c, hipStreamSynchronize(c->stream));
  return VR_OK;
}

// Measured instruction-issue ceiling (vr_bench.hip): `wavesPerSimd` blocks of 256 threads per CU
// (= that many waves on every SIMD) run `iters` passes of the chosen mix.
// out4 = {counted instructions per second, sustained clock in Hz (median over waves),
//         seconds (HIP events), counted instructions}
int vr_debug_issue_rate(vr_context *c, int kind, int wavesPerSimd, uint32_t iters, double *out4) {
  if (!c || !out4 || kind < 0 || kind > 7 || wavesPerSimd < 1 || wavesPerSimd > 8 || iters == 0)
    return fail(c, VR_E_INVALID, "vr_debug_issue_rate: bad argument");
  VR_HIP(c, hipSetDevice(c->device));
  const unsigned blocks = (unsigned)c->numCUs * (unsigned)wavesPerSimd;
  const size_t waves = (size_t)blocks * 4;
  DevBuf<unsigned long long> dOut;
  VR_HIP(c, dOut.ensure(waves * 3));
  VR_HIP(c, hipMemsetAsync(dOut.p, 0, waves * 24, c->stream));
  VR_HIP(c, launch_issue_kernel(kind, blocks, std::max<uint32_t>(iters / 16, 1), dOut.p, c->stream)); // warm-up, clocks up
  VR_HIP(c, hipEventRecord(c->ev0, c->stream));
  VR_HIP(c, launch_issue_kernel(kind, blocks, iters, dOut.p, c->stream));
  VR_HIP(c, hipEventRecord(c->ev1, c->stream));
  VR_HIP(c, hipStreamSynchronize(c->stream));
  float ms = 0.f;
  VR_HIP(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
  std::vector<unsigned long long> h(waves * 3);
  VR_HIP(c, hipMemcpy(h.data(), dOut.p, waves * 24, hipMemcpyDeviceToHost));
  std::vector<double> clk;
  for (size_t w = 0; w < waves; ++w)
    if (h[3 * w + 1])
      clk.push_back((double)h[3 * w] / (double)h[3 * w + 1] * 1e8);
  std::sort(clk.begin(), clk.end());
  const double perPass = (kind == 4 || kind == 5) ? 24.0 : 32.0;
  const double counted = (double)waves * (double)iters * perPass;
  out4[0] = counted / (ms * 1e-3);
  out4[1] = clk.empty() ? 0.0 : clk[clk.size() / 2];
  out4[2] = ms * 1e-3;
  out4[3] = counted;
  return VR_OK;
}

// the unit normals and areas of the triangle mesh in force, the caller's order (a device-resident mesh: its lazy host
// mirror, ensure_host_geometry)
int vr_debug_triangle_mesh(vr_context *c, float *normals3, float *areas, uint32_t ntris) {
  if (!c || !normals3 || !areas || c->geo.geo != 1 || ntris != c->geo.numPrims)
    return fail(c, VR_E_INVALID, "vr_debug_triangle_mesh: bad argument (a triangle geometry of ntris triangles)");
  VR_TRY(ensure_host_geometry(c));
  std::copy(c->geo.normal3.begin(), c->geo.normal3.end(), normals3);
  std::copy(c->geo.triAreas.begin(), c->geo.triAreas.end(), areas);
  return VR_OK;
}

int vr_debug_bvh_stats(vr_context *c, uint32_t *out3) {
  if (!c || !out3)
    return VR_E_INVALID;
  out3[0] = c->bvh.numNodes;
  out3[1] = c->bvh.numLeaves;
  out3[2] = c->bvh.maxDepth;
  return VR_OK;
}

} // extern "C"
