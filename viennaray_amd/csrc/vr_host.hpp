// vr_host.hpp — host-side setup of the flux tracer: bounding box, trace
// settings, boundary walls, disk neighbourhoods, areas and the (host) LBVH.
#pragma once
#include <array>
#include <cstdint>
#include <initializer_list>
#include <string>
#include <vector>

#include "vr_area.hpp"
#include "vr_types.hpp"

namespace vr {

// What the scene is: valid from the moment a geometry is set, whichever side it came from (commit_geometry, vr_api.cpp,
// is its only writer; the setters make one as {D, geo, numPrims, numVerts, gridDelta, diskRadius} and fill in the box).
struct GeometryDesc {
  int D = 3;
  int geo = 0; // 0 disk, 1 triangle
  uint32_t numPrims = 0;
  uint32_t numVerts = 0; // triangles: the mesh's vertices
  float gridDelta = 0.f, diskRadius = 0.f;
  float minC[3] = {0, 0, 0}, maxC[3] = {0, 0, 0};
};

// ... and the host's mirror of the arrays behind it.  Which array mirrors which device buffer, and who fills it:
//   disks      points3 = dPoints3 (the caller's points, the neighbourhood's input), normal3 = dNormal3, disk4 = dDisk4
//              (n x {x, y, z, r}, rayGeometryDisk.hpp:363-375)
//   triangles  verts = dVerts (numVerts x 3), tris = dTris (n x 3), normal3 = dNormal3 (unit normals), triAreas = dTriAreas
//   both       nbOff / nbIds: the neighbourhood CSR in ORIGINAL ids, lists ascending (dNbOff / dNbIds hold it in leaf order)
// A host setter (host_set_disks / host_set_triangles) fills its kind's arrays and empties the others; build_scene uploads
// them.  A device setter fills the device buffers itself (vr_context::geoOnDevice) and leaves the mirror empty until a
// host path (VR_HOST_BUILD, VR_HOST_SMOOTH, a smoothing overflow) asks for it: ensure_host_geometry then downloads the
// kind's arrays (vr_context::hostGeoValid).  nbOff / nbIds are ensure_host_neighbors' on either side.
struct HostGeometry : GeometryDesc {
  std::vector<float> disk4, normal3, points3, verts, triAreas;
  std::vector<uint32_t> tris, nbOff, nbIds;
  void clear() {
    for (std::vector<float> *v : {&disk4, &normal3, &points3, &verts, &triAreas})
      v->clear();
    for (std::vector<uint32_t> *v : {&tris, &nbOff, &nbIds})
      v->clear();
  }
};

struct Bvh {
  std::vector<float> nodes;     // 8 floats per node
  std::vector<uint32_t> order;  // leaf position -> original primitive id
  uint32_t numNodes = 0, numLeaves = 0, maxDepth = 0;
};

// the radius of every disk: the caller's, or gridDelta * DiskFactor<D> (rayTraceDisk.hpp:70 / rayUtil.hpp:99-101)
inline float host_disk_radius(float gridDelta, float radius, int D) {
  const double factor = 0.5 * (D == 3 ? 1.7320508 : 1.41421356237) * (1 + 1e-5);
  return radius > 0.f ? radius : (float)(gridDelta * factor);
}
// geometry ingestion (restates rayGeometryDisk.hpp:101-193, rayGeometryTriangle.hpp:14-88 + rayMesh.hpp:99-112)
// (they fill g's arrays and return the description: g's own stays the previous geometry's until it is committed)
GeometryDesc host_set_disks(HostGeometry &g, const float *pts, const float *nrm, uint32_t n, float gridDelta, float radius,
                            int D);
GeometryDesc host_set_triangles(HostGeometry &g, const float *verts, uint32_t nv, const uint32_t *tris, uint32_t nt,
                                float gridDelta, int D);
// Sort plane of the ray stream: rays are binned by where they cross one plane normal to
// the tracing axis, and a wavefront's rays are coherent where they HIT if that plane is
// where most first hits happen.  Estimated from the geometry alone: histogram of the
// primitives' coordinates on the axis, weighted by the area they show the source
// (r^2 |n_axis| for a disc, |Ng_axis| / 2 for a triangle); the weighted mean of the
// fullest of 256 slices.  (Only orders the work: no influence on any result.)
float host_sort_plane(const HostGeometry &g, int axis, float fallback, float *modeShare = nullptr);
// (*modeShare: the fullest slice's share of the total shown area; ~1 for a flat surface)
// rayPointNeighborhood.hpp:42-107 as a CSR (all pairs within `dist`)
void host_neighbors(int D, const float *pts3, uint32_t n, float dist, const float *minC, std::vector<uint32_t> &off,
                    std::vector<uint32_t> &ids);

// rayUtil.hpp:104-202
void host_adjust_bbox(float *lo, float *hi, int D, int direction, float pad);
std::array<int, 5> host_trace_settings(int direction);
// rayBoundary.hpp:164-245
void host_build_walls(const float *lo, const float *hi, int firstDir, int secondDir, Tri *wall);
// rayUtil.hpp:287-321
void host_orthonormal_basis(const float *v, float *basis9);
// rayGeometryDisk.hpp:266-354 (+ rayDiskBoundingBoxIntersector.hpp)
void host_disk_areas(const HostGeometry &g, const AreaParams &p, std::vector<float> &areas);

// LBVH over primitive boxes; fills bvh.nodes / bvh.order.  mortonAniso (>= 1): the Morton grid's cells have the scene
// box's proportions, but at most mortonAniso : 1 (VR_MORTON_ANISO by default)
void host_build_bvh(const HostGeometry &g, Bvh &bvh, float mortonAniso);
// leaf-ordered primitive records (vr_types.hpp)
void host_pack_prims(const HostGeometry &g, const Bvh &bvh, std::vector<float> &prims);

} // namespace vr
