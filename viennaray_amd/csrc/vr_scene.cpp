// vr_scene.cpp — the resident scene: build_scene (device LBVH, neighbourhood, quantised nodes) and the host mirrors of
// what lives on the device.
#include <algorithm>
#include <vector>

#include "vr_context.hpp"
#include "vr_planar_disks.hpp"
#include "vr_planar_lattice.hpp"

namespace vr {

// ---- scene build (device LBVH + neighbourhood; VR_HOST_BUILD=1 selects the host builder) -------
// the mirror of a device-set geometry (HostGeometry, vr_host.hpp), downloaded when a host path first reads it
int ensure_host_geometry(vr_context *c) {
  if (!c->geoOnDevice || c->hostGeoValid)
    return VR_OK;
  HostGeometry &g = c->geo;
  const size_t N = g.numPrims;
  VR_HIP(c, hipSetDevice(c->device));
  VR_HIP(c, hipStreamSynchronize(c->stream));
  auto download = [](auto &to, const auto &from, size_t n) { // (no elements: nothing to copy)
    to.resize(n);
    return n ? from.download(to.data(), n) : hipSuccess;
  };
  if (g.geo == 1) {
    VR_HIP(c, download(g.verts, c->dVerts, (size_t)g.numVerts * 3));
    VR_HIP(c, download(g.tris, c->dTris, N * 3));
    VR_HIP(c, download(g.triAreas, c->dTriAreas, N));
  } else {
    VR_HIP(c, download(g.points3, c->dPoints3, N * 3));
    VR_HIP(c, download(g.disk4, c->dDisk4, N * 4));
  }
  VR_HIP(c, download(g.normal3, c->dNormal3, N * 3));
  c->hostGeoValid = true;
  return VR_OK;
}

int ensure_host_order(vr_context *c) {
  if (c->hostOrderValid)
    return VR_OK;
  const uint32_t N = c->geo.numPrims;
  c->bvh.order.resize(N);
  VR_HIP(c, hipMemcpy(c->bvh.order.data(), c->dOrder.p, (size_t)N * 4, hipMemcpyDeviceToHost));
  c->hostOrderValid = true;
  return VR_OK;
}

// dMaterialIds holds the material ids in force: ids set from the device are there already, ids set from the host go up
// when they changed
int ensure_device_material_ids(vr_context *c) {
  if (c->materialOnDevice || !c->materialStale)
    return VR_OK;
  const std::vector<int32_t> &ids = c->materialIds;
  VR_HIP(c, hipStreamSynchronize(c->stream)); // (a kernel queued earlier may still read the previous ids)
  VR_HIP(c, c->dMaterialIds.ensure(ids.size()));
  if (!ids.empty())
    VR_HIP(c, hipMemcpy(c->dMaterialIds.p, ids.data(), ids.size() * 4, hipMemcpyHostToDevice));
  c->materialCount = (uint32_t)ids.size();
  c->materialStale = false;
  return VR_OK;
}

// dGlobalVec with room for `rows` rows of at least `stride` floats: the rows laid so far keep their values (re-laid by a
// kernel when the stride grows or the buffer moves), rows that come new read 0.  The stride only grows here; with no
// device-set vector left, upload_global_data lays everything anew at the exact stride.
int lay_global_rows(vr_context *c, uint32_t rows, uint32_t stride) {
  stride = std::max(stride, c->globalStride);
  const uint32_t kept = std::min(c->globalRowsLaid, rows);
  const size_t need = (size_t)rows * stride;
  if (stride == c->globalStride && c->dGlobalVec.p && need <= c->dGlobalVec.cap) {
    if (rows > kept)
      VR_HIP(c, hipMemsetAsync(c->dGlobalVec.p + (size_t)kept * stride, 0, (size_t)(rows - kept) * stride * 4, c->stream));
    c->globalRowsLaid = rows;
    return VR_OK;
  }
  DevBuf<float> fresh;
  VR_HIP(c, fresh.ensure(need));
  VR_HIP(c, launch_global_relayout(c->dGlobalVec.p, kept, c->globalStride, fresh.p, rows, stride, c->stream));
  VR_HIP(c, hipStreamSynchronize(c->stream)); // (the old buffer is freed below)
  c->dGlobalVec = std::move(fresh);
  c->globalStride = stride;
  c->globalRowsLaid = rows;
  return VR_OK;
}

// neighbourhood CSR in ORIGINAL ids on the host (smoothFlux, neighbour counts), lazily
int ensure_host_neighbors(vr_context *c) {
  if (c->hostNeighborsValid)
    return VR_OK;
  HostGeometry &g = c->geo;
  const uint32_t N = g.numPrims;
  if (g.geo != 0) {
    g.nbOff.assign((size_t)N + 1, 0u);
    g.nbIds.clear();
  } else if (!c->geometryDirty && c->dNbOff.p) {
    int r = ensure_host_order(c);
    if (r != VR_OK)
      return r;
    std::vector<uint32_t> off((size_t)N + 1);
    VR_HIP(c, hipMemcpy(off.data(), c->dNbOff.p, ((size_t)N + 1) * 4, hipMemcpyDeviceToHost));
    std::vector<uint32_t> ids(off[N]);
    if (off[N])
      VR_HIP(c, hipMemcpy(ids.data(), c->dNbIds.p, (size_t)off[N] * 4, hipMemcpyDeviceToHost));
    g.nbOff.assign((size_t)N + 1, 0u);
    for (uint32_t q = 0; q < N; ++q)
      g.nbOff[c->bvh.order[q] + 1] = off[q + 1] - off[q];
    for (uint32_t i = 0; i < N; ++i)
      g.nbOff[i + 1] += g.nbOff[i];
    g.nbIds.resize(off[N]);
    for (uint32_t q = 0; q < N; ++q) {
      uint32_t w = g.nbOff[c->bvh.order[q]];
      for (uint32_t j = off[q]; j < off[q + 1]; ++j)
        g.nbIds[w++] = c->bvh.order[ids[j]];
      std::sort(g.nbIds.begin() + g.nbOff[c->bvh.order[q]], g.nbIds.begin() + w);
    }
  } else {
    int r = ensure_host_geometry(c);
    if (r != VR_OK)
      return r;
    host_neighbors(g.D, g.points3.data(), N, 2 * g.diskRadius, g.minC, g.nbOff, g.nbIds);
  }
  c->hostNeighborsValid = true;
  return VR_OK;
}

// 16-byte nodes for the per-lane traversal: frame from the root box (which holds every
// padded primitive box), two cells of margin so the outward rounding never clamps
static int quantize_scene(vr_context *c, const float *preNodes, const float *root8) {
  const float lo[3] = {root8[0], root8[1], root8[2]}, hi[3] = {root8[4], root8[5], root8[6]};
  for (int k = 0; k < 3; ++k) {
    c->sceneLo[k] = lo[k];
    c->sceneHi[k] = hi[k];
    const float ext = hi[k] - lo[k];
    c->qscale[k] = ext > 0.f ? 65531.0f / ext : 0.f;
    c->qbase[k] = ext > 0.f ? lo[k] - 2.0f / c->qscale[k] : lo[k];
  }
  VR_HIP(c, c->dQNodes.ensure((size_t)c->numNodes * 4));
  VR_HIP(c, c->dPNodes.ensure((size_t)std::max<uint32_t>(c->numNodes, 1u) * 8));
  VR_HIP(c, launch_quantize_nodes(preNodes, c->numNodes, c->qbase, c->qscale, c->dQNodes.p, c->dPNodes.p, c->stream));
  VR_HIP(c, hipStreamSynchronize(c->stream));
  return VR_OK;
}

// Uniform disks (vr_context::uniformDisks, planarDisks): the reduction over the packed disk records on the stream, its
// words on their way into `words`; the caller's next synchronisation of the stream delivers them, set_uniform_disks files them.
static int read_uniform_disks(vr_context *c, uint32_t (&words)[VR_UNIFORM_WORDS]) {
  VR_HIP(c, c->dUniformDisks.ensure(VR_UNIFORM_WORDS));
  VR_HIP(c, launch_uniform_disks(c->dPrims.p, c->geo.numPrims, c->dUniformDisks.p, c->stream));
  VR_HIP(c, hipMemcpyAsync(words, c->dUniformDisks.p, sizeof(words), hipMemcpyDeviceToHost, c->stream));
  return VR_OK;
}
static void set_uniform_disks(vr_context *c, const uint32_t (&words)[VR_UNIFORM_WORDS]) {
  c->uniformDisks = words[0] == 0u && c->geo.geo == 0 && c->geo.numPrims > 0; // (a mesh: nothing was launched)
  for (int k = 0; k < 4; ++k)
    c->uniformWords[k] = words[1 + k];
  // planar as well: the shared normal is +-1 along one axis and +-0 along the others (the rule of vr_planar_disks.hpp),
  // every centre carries one word in that coordinate, every centre coordinate is finite
  const uint32_t nw[3] = {words[1], words[2], words[3]};
  const int axis = planar_disk_axis(nw);
  c->planarDisks = c->uniformDisks && axis >= 0 && words[5 + axis] == 0u && words[8] == 0u;
  c->planarAxis = c->planarDisks ? axis : 0;
  c->planarWord = c->planarDisks ? words[9 + axis] : 0u;
}

// Lattice cloud (vr_context::planarLattice, vr_planar_lattice.hpp): where the planar cloud's extent fits a table, one kernel
// over the records in their NEW leaf order validates and fills it, and one word read back decides.  Called at the end of
// every device build — the table holds leaf positions — behind set_uniform_disks; synchronises the stream.
static int build_lattice_table(vr_context *c) {
  c->planarLattice = false;
  const HostGeometry &g = c->geo;
  if (!c->planarDisks || g.D != 3 || !c->haveWide)
    return VR_OK;
  int b1, b2;
  planar_in_plane_axes(c->planarAxis, b1, b2);
  const int n1 = lattice_axis_points(g.minC[b1], g.maxC[b1], g.gridDelta), n2 = lattice_axis_points(g.minC[b2], g.maxC[b2], g.gridDelta);
  if (!lattice_table_fits(n1, n2, g.numPrims))
    return VR_OK;
  const size_t cells = (size_t)n1 * (size_t)n2;
  VR_HIP(c, c->dLattice.ensure(cells + 1));
  VR_HIP(c, launch_lattice_table(c->dPrims.p, g.numPrims, b1, b2, g.minC[b1], g.minC[b2], 1.f / g.gridDelta, n1, n2, c->dLattice.p, c->stream));
  uint32_t flag = 1u;
  VR_HIP(c, hipMemcpyAsync(&flag, c->dLattice.p + cells, 4, hipMemcpyDeviceToHost, c->stream));
  VR_HIP(c, hipStreamSynchronize(c->stream));
  c->planarLattice = flag == 0u;
  c->latticeN[0] = n1;
  c->latticeN[1] = n2;
  c->latticePhase[0] = g.minC[b1];
  c->latticePhase[1] = g.minC[b2];
  return VR_OK;
}

int build_scene(vr_context *c) {
  const Knobs &K = c->knobs;
  HostGeometry &g = c->geo;
  const uint32_t N = g.numPrims;
  const bool disk = g.geo == 0;
  c->hostOrderValid = false;
  c->hostNeighborsValid = false;
  VR_HIP(c, c->dLeafOfOrig.ensure(N));
  VR_HIP(c, c->dOrder.ensure(N));
  {
    uint32_t R = 1;
    if (K.accReplicas)
      R = *K.accReplicas;
    else
      while (R < 64u && (size_t)N * (2u * R) <= (1u << 21))
        R *= 2u;
    while (R & (R - 1u)) // power of two
      R &= R - 1u;
    c->accReplicas = R;
    c->accStride = (N + 15u) & ~15u; // replicas start on 128-byte lines
    c->accPlanes = 0;                // (buffers are sized per data label in vr_apply_prepare)
  }
  VR_HIP(c, c->dCounters.ensure(C_BLOCK));
  VR_HIP(c, c->dNbOff.ensure((size_t)N + 1));
  if (K.hostBuild) {
    // host builder (validation path): LBVH + CSR on the CPU, uploaded
    {
      const int r = ensure_host_geometry(c);
      if (r != VR_OK)
        return r;
    }
    if (disk)
      host_neighbors(g.D, g.points3.data(), N, 2 * g.diskRadius, g.minC, g.nbOff, g.nbIds);
    else
      g.nbOff.assign((size_t)N + 1, 0u), g.nbIds.clear();
    c->hostNeighborsValid = true;
    host_build_bvh(g, c->bvh, K.mortonAniso);
    c->hostOrderValid = true;
    std::vector<float> prims;
    host_pack_prims(g, c->bvh, prims);
    c->leafOfOrig.resize(N);
    for (uint32_t q = 0; q < N; ++q)
      c->leafOfOrig[c->bvh.order[q]] = q;
    std::vector<uint32_t> off((size_t)N + 1, 0u), ids(g.nbIds.size());
    for (uint32_t q = 0; q < N; ++q) {
      const uint32_t o = c->bvh.order[q];
      off[q + 1] = off[q] + (g.nbOff[o + 1] - g.nbOff[o]);
    }
    for (uint32_t q = 0; q < N; ++q) {
      const uint32_t o = c->bvh.order[q];
      uint32_t w = off[q];
      for (uint32_t j = g.nbOff[o]; j < g.nbOff[o + 1]; ++j)
        ids[w++] = c->leafOfOrig[g.nbIds[j]];
    }
    VR_HIP(c, c->dNodes.ensure(c->bvh.nodes.size()));
    VR_HIP(c, c->dPrims.ensure(prims.size()));
    VR_HIP(c, c->dNbIds.ensure(ids.size()));
    c->nbTotal = (uint32_t)ids.size();
    VR_HIP(c, hipMemcpyAsync(c->dNodes.p, c->bvh.nodes.data(), c->bvh.nodes.size() * 4, hipMemcpyHostToDevice, c->stream));
    VR_HIP(c, hipMemcpyAsync(c->dPrims.p, prims.data(), prims.size() * 4, hipMemcpyHostToDevice, c->stream));
    VR_HIP(c, hipMemcpyAsync(c->dNbOff.p, off.data(), off.size() * 4, hipMemcpyHostToDevice, c->stream));
    if (!ids.empty())
      VR_HIP(c, hipMemcpyAsync(c->dNbIds.p, ids.data(), ids.size() * 4, hipMemcpyHostToDevice, c->stream));
    VR_HIP(c, hipMemcpyAsync(c->dLeafOfOrig.p, c->leafOfOrig.data(), (size_t)N * 4, hipMemcpyHostToDevice, c->stream));
    VR_HIP(c, hipMemcpyAsync(c->dOrder.p, c->bvh.order.data(), (size_t)N * 4, hipMemcpyHostToDevice, c->stream));
    uint32_t uni[VR_UNIFORM_WORDS] = {};
    if (disk) // (the same pass over the resident records as behind the device builder)
      VR_TRY(read_uniform_disks(c, uni));
    VR_HIP(c, hipStreamSynchronize(c->stream));
    set_uniform_disks(c, uni);
    c->numNodes = c->bvh.numNodes;
    c->haveWide = false; // (validation path: walks only)
    c->planarLattice = false; // (... and no packet query to look candidates up for)
    return quantize_scene(c, c->dNodes.p, c->bvh.nodes.data()); // (host builder: pre-order already)
  }

  // ---- device builder ----
  SetupParams s{};
  // (triangles: a leaf of up to 3 — their test is 64 bytes and ~60 instructions per primitive; measured 4 -> 3:
  //  trenchMesh 0.1 29.6 -> 28.4 ms, C4 21.4 -> 20.6; disks: 2 .. 4 within 2 %, 6 and 8 slower)
  s.leafMax = K.leafMax.value_or(g.geo == 1 ? 3u : (uint32_t)VR_LEAF_MAX);
  s.orderAxis = c->ts[0];                                  // rays travel along this axis ...
  s.orderSign = K.noChildOrder ? 0.f : c->ts[3] ? 1.f : -1.f; // ... from its max (min) side: that child first
  s.n = N;
  s.geo = g.geo;
  s.D = g.D;
  s.nbDist = 2 * g.diskRadius;
  s.mortonAniso = K.mortonAniso;
  if (c->geoOnDevice) {
    // (vr_set_disks_device left dPoints3 / dNormal3 / dDisk4 filled, vr_set_triangles_device dVerts / dTris / dNormal3:
    //  nothing to upload)
  } else if (disk) {
    VR_HIP(c, c->dNormal3.ensure((size_t)N * 3));
    VR_HIP(c, hipMemcpyAsync(c->dNormal3.p, g.normal3.data(), (size_t)N * 12, hipMemcpyHostToDevice, c->stream));
    VR_HIP(c, c->dDisk4.ensure((size_t)N * 4));
    VR_HIP(c, c->dPoints3.ensure((size_t)N * 3));
    VR_HIP(c, hipMemcpyAsync(c->dPoints3.p, g.points3.data(), (size_t)N * 12, hipMemcpyHostToDevice, c->stream));
    VR_HIP(c, launch_disk4(c->dPoints3.p, N, g.diskRadius, g.D, c->dDisk4.p, c->stream)); // (= g.disk4, made on the device)
  } else {
    VR_HIP(c, c->dNormal3.ensure((size_t)N * 3));
    VR_HIP(c, hipMemcpyAsync(c->dNormal3.p, g.normal3.data(), (size_t)N * 12, hipMemcpyHostToDevice, c->stream));
    VR_HIP(c, c->dVerts.ensure(g.verts.size()));
    VR_HIP(c, c->dTris.ensure(g.tris.size()));
    VR_HIP(c, hipMemcpyAsync(c->dVerts.p, g.verts.data(), g.verts.size() * 4, hipMemcpyHostToDevice, c->stream));
    VR_HIP(c, hipMemcpyAsync(c->dTris.p, g.tris.data(), g.tris.size() * 4, hipMemcpyHostToDevice, c->stream));
  }
  const size_t tiles = ((size_t)N + 1023) / 1024;
  VR_HIP(c, c->dBox.ensure((size_t)N * 6));
  VR_HIP(c, c->dSBox.ensure((size_t)N * 6));
  VR_HIP(c, c->dNodeBox.ensure((size_t)N * 6));
  VR_HIP(c, c->dBounds.ensure(8));
  VR_HIP(c, c->dKeysA.ensure(N));
  VR_HIP(c, c->dKeysB.ensure(N));
  VR_HIP(c, c->dValsA.ensure(N));
  VR_HIP(c, c->dValsB.ensure(N));
  VR_HIP(c, c->dSortTable.ensure(256 * tiles));
  VR_HIP(c, c->dRangeLo.ensure(N));
  VR_HIP(c, c->dRangeHi.ensure(N));
  VR_HIP(c, c->dChildL.ensure(N));
  VR_HIP(c, c->dChildR.ensure(N));
  VR_HIP(c, c->dParentInt.ensure(N));
  VR_HIP(c, c->dParentLeaf.ensure(N));
  VR_HIP(c, c->dArrive.ensure(N));
  VR_HIP(c, c->dSubSize.ensure(N));
  VR_HIP(c, c->dNodes.ensure(((size_t)2 * N) * 8));
  VR_HIP(c, c->dNodesPre.ensure(((size_t)2 * N) * 8));
  VR_HIP(c, c->dPrims.ensure((size_t)N * (disk ? 8 : 16)));
  VR_HIP(c, c->dScanTmp.ensure(2 * ((256 * tiles + (size_t)N + 1) / 2048 + 4) + 64));
  s.disk4 = c->dDisk4.p;
  s.normal3 = c->dNormal3.p;
  s.points3 = c->dPoints3.p;
  s.verts = c->dVerts.p;
  s.tris = c->dTris.p;
  s.box = c->dBox.p;
  s.sbox = c->dSBox.p;
  s.bounds = c->dBounds.p;
  s.keysA = c->dKeysA.p;
  s.keysB = c->dKeysB.p;
  s.valsA = c->dValsA.p;
  s.valsB = c->dValsB.p;
  s.sortTable = c->dSortTable.p;
  s.rangeLo = c->dRangeLo.p;
  s.rangeHi = c->dRangeHi.p;
  s.childL = c->dChildL.p;
  s.childR = c->dChildR.p;
  s.parentInt = c->dParentInt.p;
  s.parentLeaf = c->dParentLeaf.p;
  s.arrive = c->dArrive.p;
  s.nodeBox = c->dNodeBox.p;
  s.subSize = c->dSubSize.p;
  s.nodes = c->dNodes.p;
  s.nodesPre = c->dNodesPre.p;
  s.prims = c->dPrims.p;
  s.leafOfOrig = c->dLeafOfOrig.p;
  s.order = c->dOrder.p;
  s.nbOff = c->dNbOff.p;
  s.nbIds = nullptr;
  VR_HIP(c, c->dWide.ensure(wide_tree_entries(N) * 8));
  s.wide = c->dWide.p;
  VR_HIP(c, launch_setup_bvh(s, c->dScanTmp.p, c->stream));
  VR_HIP(c, launch_wide_tree(s, c->wideRoot, c->stream));
  c->haveWide = true;
  // every build is verified (one small kernel; its counter is read back with the syncs below):
  // the fit's cross-workgroup hand-over is the one place the build relies on memory ordering
  VR_HIP(c, hipMemsetAsync(c->dBounds.p + 6, 0, 4, c->stream));
  VR_HIP(c, launch_bvh_check(s, c->dBounds.p + 6, c->stream));
  c->lastSetup = s;
  c->haveSetup = true;
  if (disk) {
    // neighbourhood: ONE query that counts and keeps up to VR_NB_KEEP ids per primitive -> scan -> pack (the query, a
    // range walk of the BVH per primitive, is the most expensive kernel of a build: 0.4 ms per 10^6 disks; counting and
    // filling in two passes walked twice).  A primitive with more neighbours: the two-pass path.
    VR_HIP(c, c->dNbTmp.ensure((size_t)N * VR_NB_KEEP + 1));
    s.nbTmp = c->dNbTmp.p;
    VR_HIP(c, hipMemsetAsync(c->dNbTmp.p + (size_t)N * VR_NB_KEEP, 0, 4, c->stream));
    VR_HIP(c, hipMemsetAsync(c->dNbOff.p + N, 0, 4, c->stream));
    VR_HIP(c, launch_setup_neighbors(s, 2, c->stream));
    VR_HIP(c, launch_scan(c->dNbOff.p, N + 1, c->dScanTmp.p, c->stream));
    uint32_t total = 0, overflow = 0;
    VR_HIP(c, hipMemcpyAsync(&total, c->dNbOff.p + N, 4, hipMemcpyDeviceToHost, c->stream));
    VR_HIP(c, hipMemcpyAsync(&overflow, c->dNbTmp.p + (size_t)N * VR_NB_KEEP, 4, hipMemcpyDeviceToHost, c->stream));
    VR_HIP(c, hipStreamSynchronize(c->stream));
    VR_HIP(c, c->dNbIds.ensure(total));
    c->nbTotal = total;
    s.nbIds = c->dNbIds.p;
    VR_HIP(c, launch_setup_neighbors(s, (overflow || K.nbTwoPass) ? 1 : 3, c->stream));
  } else {
    c->nbTotal = 0;
    VR_HIP(c, hipMemsetAsync(c->dNbOff.p, 0, ((size_t)N + 1) * 4, c->stream));
    VR_HIP(c, c->dNbIds.ensure(1));
  }
  float root8[8];
  uint32_t sz = 0, bad = 0;
  uint32_t uni[VR_UNIFORM_WORDS] = {};
  if (disk) // (the packed records never change behind launch_setup_bvh: a re-fit below leaves them as they are)
    VR_TRY(read_uniform_disks(c, uni));
  VR_HIP(c, hipMemcpyAsync(root8, c->dNodesPre.p, sizeof(root8), hipMemcpyDeviceToHost, c->stream));
  VR_HIP(c, hipMemcpyAsync(&sz, c->dSubSize.p, 4, hipMemcpyDeviceToHost, c->stream));
  VR_HIP(c, hipMemcpyAsync(&bad, c->dBounds.p + 6, 4, hipMemcpyDeviceToHost, c->stream));
  VR_HIP(c, hipStreamSynchronize(c->stream));
  set_uniform_disks(c, uni);
  c->bvhRefits = 0;
  if (bad != 0) {
    // never observed; the textbook agent-scope fences cost 3 ms per 10^6 primitives
    s.strictFence = 1;
    s.nbIds = nullptr;
    VR_HIP(c, launch_fit_bvh(s, c->stream));
    VR_HIP(c, hipMemsetAsync(c->dBounds.p + 6, 0, 4, c->stream));
    VR_HIP(c, launch_bvh_check(s, c->dBounds.p + 6, c->stream));
    VR_HIP(c, hipMemcpyAsync(root8, c->dNodesPre.p, sizeof(root8), hipMemcpyDeviceToHost, c->stream));
    VR_HIP(c, hipMemcpyAsync(&sz, c->dSubSize.p, 4, hipMemcpyDeviceToHost, c->stream));
    VR_HIP(c, hipMemcpyAsync(&bad, c->dBounds.p + 6, 4, hipMemcpyDeviceToHost, c->stream));
    VR_HIP(c, hipStreamSynchronize(c->stream));
    c->bvhRefits = 1;
    if (bad != 0)
      return fail(c, VR_E_HIP, "device BVH build failed its consistency check twice");
    if (disk) { // the neighbourhood was queried on the inconsistent tree: redo it
      s.nbIds = nullptr;
      VR_HIP(c, hipMemsetAsync(c->dNbOff.p + N, 0, 4, c->stream));
      VR_HIP(c, launch_setup_neighbors(s, 0, c->stream));
      VR_HIP(c, launch_scan(c->dNbOff.p, N + 1, c->dScanTmp.p, c->stream));
      uint32_t total = 0;
      VR_HIP(c, hipMemcpyAsync(&total, c->dNbOff.p + N, 4, hipMemcpyDeviceToHost, c->stream));
      VR_HIP(c, hipStreamSynchronize(c->stream));
      VR_HIP(c, c->dNbIds.ensure(total));
      c->nbTotal = total;
      s.nbIds = c->dNbIds.p;
      VR_HIP(c, launch_setup_neighbors(s, 1, c->stream));
      VR_HIP(c, hipStreamSynchronize(c->stream));
    }
    c->lastSetup = s;
  }
  c->numNodes = sz & 0x7FFFFFFFu;
  c->bvh.numNodes = c->numNodes;
  c->bvh.numLeaves = 0;
  c->bvh.maxDepth = 0;
  const int rq = quantize_scene(c, c->dNodesPre.p, root8);
  c->dNodesPre.release(); // (build-time scratch)
  if (rq != VR_OK)
    return rq;
  return build_lattice_table(c); // (the records' order is final: a re-fit above leaves it as it is)
}

} // namespace vr
