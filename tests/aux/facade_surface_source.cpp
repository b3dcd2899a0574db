// Compile-only check of the façade's surface source (gpu/raygTrace.hpp:267-297 of the reference): setSurfaceSource and
// clearSurfaceSource with the reference's names and argument types on TraceDisk and TraceTriangle.
#include <rayTraceDisk.hpp>
#include <rayTraceTriangle.hpp>

#include <vector>

using namespace viennaray;

template <class Tracer> static void use(Tracer &tracer) {
  const std::vector<Vec3D<float>> positions{{0.f, 0.f, 0.f}, {1.f, 0.f, 0.f}};
  const std::vector<Vec3D<float>> normals{{0.f, 0.f, 1.f}, {0.f, 0.f, 2.f}};
  const std::vector<float> weights{1.f, 0.5f};
  tracer.setSurfaceSource(positions, normals, weights, 4.f, 1e-4f);
  tracer.clearSurfaceSource();
}

int main() {
  TraceDisk<float, 3> disks;
  TraceTriangle<float, 3> triangles;
  use(disks);
  use(triangles);
  return 0;
}
