// viennaray.hpp — header-only C++ façade with the reference's class, method and
// enum names for the accelerated path, implemented on the C ABI of
// include/viennaray_amd.h (link with libviennaray_amd.so).
//
// It mirrors, for the path Trace<T,D>::apply() covers:
//   viennaray::Trace / TraceDisk / TraceTriangle   (rayTrace.hpp:15-180,
//       rayTraceDisk.hpp:13-224, rayTraceTriangle.hpp:13-154)
//   viennaray::DiffuseParticle / SpecularParticle  (rayParticle.hpp:126-204)
//   viennaray::TracingData                         (rayTracingData.hpp:16-219)
//   viennaray::TraceInfo, BoundaryCondition, TraceDirection, NormalizationType
//   viennaray::DiskMesh / TriangleMesh             (rayMesh.hpp:82-131)
//   rayInternal::readGridFromFile / readMeshFromFile / createPlaneGrid / writeVTK / writeVTP
//   LineMesh + convertLinesToTriangles (rayMesh.hpp)
// so a reference example builds by pointing its include path here (see
// examples/ and INTEGRATION.md).  The device computes in float; NumericType
// double is accepted and converted at the boundary, as the reference does when
// it fills Embree's float buffers (rayGeometryDisk.hpp:137-175).
//
// Particles and sources.  AbstractParticle / Particle<Derived> / Source carry the reference's
// virtual interfaces (rayParticle.hpp:21-122, raySource.hpp:10-19), so user classes compile
// unchanged.  What runs on the device is decided by AbstractParticle::deviceModel(): the
// built-in particles (and the plug-ins of viennaray_amd/csrc/vr_particles.hpp) describe
// themselves as a vr_particle POD; a user particle whose per-hit logic exists only as host
// virtuals cannot be called from a HIP kernel — apply() reports that instead of tracing
// something else, and the way in is a model in the device registry plus a deviceModel()
// override.  Sources: SourceGrid runs natively in the generator kernel; any other Source is
// evaluated on the host once per ray (getOriginAndDirection with a counting stand-in of the
// per-ray engine) and the rays are handed to the device, which continues each ray's random
// stream where the callback left it.
#pragma once

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <fstream>
#include <functional>
#include <iostream>
#include <limits>
#include <memory>
#include <random>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

// (the reference's headers pull in OpenMP: programs written against them call omp_set_num_threads() without
//  including <omp.h> themselves — tests/traceInterface/traceInterface.cpp:27, tests/rngSeed/rngSeed.cpp:10)
#if defined(_OPENMP) && __has_include(<omp.h>)
#include <omp.h>
#endif

#include "../viennaray_amd.h"

namespace viennacore {
template <class T, size_t D> using VectorType = std::array<T, D>;
template <class T> using Vec2D = std::array<T, 2>;
template <class T> using Vec3D = std::array<T, 3>;
using Vec3Df = Vec3D<float>;
using Vec3Dd = Vec3D<double>;

// The handful of ViennaCore vector helpers (vcVectorType.hpp) that ViennaRay programs use on
// their points and normals, so that such a program builds without ViennaCore.  Plain
// component loops; known answers: the reference's tests/utilFuncs (tests/aux/facade_units.cpp).
template <class T, size_t D> VectorType<T, D> operator+(const VectorType<T, D> &a, const VectorType<T, D> &b) {
  VectorType<T, D> r;
  for (size_t i = 0; i < D; ++i)
    r[i] = a[i] + b[i];
  return r;
}
template <class T, size_t D> VectorType<T, D> operator-(const VectorType<T, D> &a, const VectorType<T, D> &b) {
  VectorType<T, D> r;
  for (size_t i = 0; i < D; ++i)
    r[i] = a[i] - b[i];
  return r;
}
template <class T, size_t D> VectorType<T, D> operator*(const T &f, const VectorType<T, D> &a) {
  VectorType<T, D> r;
  for (size_t i = 0; i < D; ++i)
    r[i] = f * a[i];
  return r;
}
template <class T, size_t D> VectorType<T, D> operator*(const VectorType<T, D> &a, const T &f) { return f * a; }
template <class T, size_t D>
VectorType<T, D> Sum(const VectorType<T, D> &a, const VectorType<T, D> &b, const VectorType<T, D> &c) {
  return a + b + c;
}
template <class T, size_t D> T DotProduct(const VectorType<T, D> &a, const VectorType<T, D> &b) {
  T s = 0;
  for (size_t i = 0; i < D; ++i)
    s += a[i] * b[i];
  return s;
}
template <class T> Vec3D<T> CrossProduct(const Vec3D<T> &a, const Vec3D<T> &b) {
  return Vec3D<T>{a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
}
template <class T, size_t D> T Norm2(const VectorType<T, D> &a) { return DotProduct(a, a); }
template <class T, size_t D> T Norm(const VectorType<T, D> &a) { return std::sqrt(Norm2(a)); }
template <class T, size_t D> void Normalize(VectorType<T, D> &a) {
  const T n = Norm(a);
  if (n > T(0))
    for (size_t i = 0; i < D; ++i)
      a[i] /= n;
}
// (ViennaCore has both forms: in place for an lvalue, a normalised copy for a const / temporary argument —
//  tests/smoothing/smoothing.cpp:26 uses the second)
template <class T, size_t D> VectorType<T, D> Normalize(const VectorType<T, D> &a) {
  VectorType<T, D> r = a;
  Normalize(r);
  return r;
}
template <class T, size_t D> bool IsNormalized(const VectorType<T, D> &a) {
  return std::fabs(Norm(a) - T(1)) < T(1e-4);
}
template <class T, size_t D> T Distance(const VectorType<T, D> &a, const VectorType<T, D> &b) { return Norm(a - b); }
template <class T, size_t D> VectorType<T, D> Inv(const VectorType<T, D> &a) { return T(-1) * a; }
template <class T, size_t D>
VectorType<T, D> ScaleAdd(const VectorType<T, D> &a, const VectorType<T, D> &b, const T &f) { // a * f + b
  return f * a + b;
}
template <class T> Vec3D<T> ComputeNormal(const Vec3D<Vec3D<T>> &p) { return CrossProduct(p[1] - p[0], p[2] - p[0]); }

// vcLogger.hpp: the part ViennaRay programs touch (examples/triangle3D/triangle3D.cpp:14:
// Logger::setLogLevel(LogLevel::DEBUG)).  Messages at or below the current level go to std::cout / std::cerr;
// nothing here aborts.
enum class LogLevel : unsigned { ERROR = 0, WARNING = 1, INFO = 2, INTERMEDIATE = 3, TIMING = 4, DEBUG = 5 };
class Logger {
  std::string pending_;
  bool toError_ = false;
  static LogLevel &level() {
    static LogLevel l = LogLevel::INFO;
    return l;
  }
  Logger() = default;
  Logger &add(LogLevel l, const char *tag, const std::string &msg, bool err) {
    if (static_cast<unsigned>(level()) >= static_cast<unsigned>(l)) {
      pending_ += std::string("\n    ") + tag + msg + "\n";
      toError_ = toError_ || err;
    }
    return *this;
  }

public:
  Logger(const Logger &) = delete;
  Logger &operator=(const Logger &) = delete;
  static Logger &getInstance() {
    static Logger instance;
    return instance;
  }
  static void setLogLevel(LogLevel l) { level() = l; }
  static LogLevel getLogLevel() { return level(); }
  Logger &addDebug(const std::string &s) { return add(LogLevel::DEBUG, "DEBUG: ", s, false); }
  Logger &addTiming(const std::string &s, double seconds) {
    return add(LogLevel::TIMING, "", s + ": " + std::to_string(seconds) + " s", false);
  }
  Logger &addInfo(const std::string &s) { return add(LogLevel::INFO, "", s, false); }
  Logger &addWarning(const std::string &s) { return add(LogLevel::WARNING, "WARNING: ", s, false); }
  Logger &addError(const std::string &s, bool = true) { return add(LogLevel::ERROR, "ERROR: ", s, true); }
  void print(std::ostream &out = std::cout) {
    (toError_ ? std::cerr : out) << pending_;
    pending_.clear();
    toError_ = false;
  }
};

// vcRNG.hpp: viennacore::RNG is std::mt19937_64.  Here a thin wrapper with the same
// UniformRandomBitGenerator interface that also counts the outputs drawn: a host-side Source
// callback consumes part of a ray's random stream and the device continues after it.
struct RNG {
  using result_type = std::mt19937_64::result_type;
  std::mt19937_64 engine;
  uint64_t draws = 0;
  RNG() = default;
  explicit RNG(result_type seed) : engine(seed) {}
  void seed(result_type s) {
    engine.seed(s);
    draws = 0;
  }
  static constexpr result_type min() { return std::mt19937_64::min(); }
  static constexpr result_type max() { return std::mt19937_64::max(); }
  result_type operator()() {
    ++draws;
    return engine();
  }
};

// vcRNG.hpp tea<N>: the per-ray seed hash (rayTraceKernel.hpp:120)
template <unsigned N> inline unsigned tea(unsigned v0, unsigned v1) {
  unsigned s0 = 0;
  for (unsigned n = 0; n < N; ++n) {
    s0 += 0x9e3779b9u;
    v0 += ((v1 << 4) + 0xa341316cu) ^ (v1 + s0) ^ ((v1 >> 5) + 0xc8013ea4u);
    v1 += ((v0 << 4) + 0xad90777du) ^ (v0 + s0) ^ ((v0 >> 5) + 0x7e95761eu);
  }
  return v0;
}

struct Timer {
  std::chrono::steady_clock::time_point t0;
  long long currentDuration = 0; // ns
  void start() { t0 = std::chrono::steady_clock::now(); }
  void finish() {
    currentDuration = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
  }
};
} // namespace viennacore

namespace viennaray {
using namespace viennacore;

enum class BoundaryCondition : unsigned { REFLECTIVE_BOUNDARY = 0, PERIODIC_BOUNDARY = 1, IGNORE_BOUNDARY = 2 };
enum class TraceDirection : unsigned { POS_X = 0, NEG_X = 1, POS_Y = 2, NEG_Y = 3, POS_Z = 4, NEG_Z = 5 };
enum class NormalizationType : unsigned { SOURCE = 0, MAX = 1 };
enum class TracingDataMergeEnum : unsigned { SUM = 0, APPEND = 1, AVERAGE = 2 };

struct TraceInfo {
  size_t numRays = 0;
  size_t totalRaysTraced = 0;
  size_t nonGeometryHits = 0;
  size_t geometryHits = 0;
  size_t particleHits = 0;
  size_t boundaryHits = 0;
  size_t reflections = 0;
  double time = 0.0;
  bool warning = false;
  bool error = false;
};

// ---- meshes (rayMesh.hpp) -------------------------------------------------------
struct DiskMesh {
  DiskMesh() = default;
  DiskMesh(const std::vector<Vec3Df> &pts, const std::vector<Vec3Df> &nms, float delta)
      : nodes(pts), normals(nms), gridDelta(delta) {}
  std::vector<Vec3Df> nodes;
  std::vector<Vec3Df> normals;
  float gridDelta = 0.f;
};

struct TriangleMesh {
  TriangleMesh() = default;
  TriangleMesh(std::vector<Vec3Df> const &pts, std::vector<Vec3D<unsigned>> const &tris, float delta)
      : nodes(pts), triangles(tris), gridDelta(delta) {}
  std::vector<Vec3Df> nodes;
  std::vector<Vec3D<unsigned>> triangles;
  float gridDelta = 0.f;
};

// rayMesh.hpp:27-80: 2-D surface as line segments; zero-length segments are dropped
struct LineMesh {
  LineMesh() = default;
  LineMesh(const std::vector<Vec3Df> &pts, const std::vector<Vec2D<unsigned>> &lns, float delta)
      : nodes(pts), gridDelta(delta) {
    for (auto const &l : lns) {
      const auto &p0 = nodes[l[0]];
      const auto &p1 = nodes[l[1]];
      const float dx = p1[0] - p0[0], dy = p1[1] - p0[1], dz = p1[2] - p0[2];
      if (std::sqrt(dx * dx + dy * dy + dz * dz) > 1e-6f)
        lines.push_back(l);
    }
  }
  std::vector<Vec3Df> nodes;
  std::vector<Vec2D<unsigned>> lines;
  float gridDelta = 0.f;
};

// rayMesh.hpp:133-175: every line becomes a strip of two triangles of height gridDelta
// (z = +-gridDelta/2); node 2i is node i at +z, node 2i+1 at -z
inline TriangleMesh convertLinesToTriangles(const LineMesh &lineMesh) {
  TriangleMesh mesh;
  mesh.gridDelta = lineMesh.gridDelta;
  const float w2 = lineMesh.gridDelta * 0.5f;
  mesh.nodes.reserve(lineMesh.nodes.size() * 2);
  for (auto const &p : lineMesh.nodes) {
    mesh.nodes.push_back(Vec3Df{p[0], p[1], w2});
    mesh.nodes.push_back(Vec3Df{p[0], p[1], -w2});
  }
  mesh.triangles.reserve(lineMesh.lines.size() * 2);
  for (auto const &line : lineMesh.lines) {
    const unsigned p0 = line[0] * 2, p1 = line[1] * 2;
    mesh.triangles.push_back(Vec3D<unsigned>{p0, p1, p0 + 1});
    mesh.triangles.push_back(Vec3D<unsigned>{p0 + 1, p1, p1 + 1});
  }
  return mesh;
}

// ---- TracingData (rayTracingData.hpp:16-219) ---------------------------------------------
// Labelled per-primitive vectors and labelled scalars with a merge type each.  The device
// path fills vector 0 of Trace::getLocalData() (merge type SUM); everything else is a plain
// container for the caller, with the reference's method names and defaults.
template <typename NumericType> class TracingData {
  std::vector<NumericType> scalars_;
  std::vector<std::vector<NumericType>> vectors_;
  std::vector<std::string> scalarLabels_, vectorLabels_;
  std::vector<TracingDataMergeEnum> scalarMerge_, vectorMerge_;

  static int find(const std::vector<std::string> &labels, const std::string &label, const char *what) {
    for (int i = 0; i < (int)labels.size(); ++i)
      if (labels[i] == label)
        return i;
    std::cerr << "Can not find " << what << " data label in TracingData.\n";
    return -1;
  }

public:
  TracingData() = default;
  TracingData(const TracingData &) = default;
  TracingData &operator=(const TracingData &) = default;
  // a moved-from object is left EMPTY (the reference's test checks data() == nullptr)
  TracingData(TracingData &&o) noexcept { *this = std::move(o); }
  TracingData &operator=(TracingData &&o) noexcept {
    scalars_ = std::exchange(o.scalars_, {});
    vectors_ = std::exchange(o.vectors_, {});
    scalarLabels_ = std::exchange(o.scalarLabels_, {});
    vectorLabels_ = std::exchange(o.vectorLabels_, {});
    scalarMerge_ = std::exchange(o.scalarMerge_, {});
    vectorMerge_ = std::exchange(o.vectorMerge_, {});
    return *this;
  }

  void setNumberOfVectorData(int size) {
    vectors_.clear();
    vectors_.resize(size);
    vectorMerge_.resize(size, TracingDataMergeEnum::SUM);
    vectorLabels_.resize(size, "vectorData");
  }
  void setNumberOfScalarData(int size) {
    scalars_.clear();
    scalars_.resize(size);
    scalarMerge_.resize(size, TracingDataMergeEnum::SUM);
    scalarLabels_.resize(size, "scalarData");
  }
  void setScalarData(int num, NumericType value, std::string label = "scalarData") {
    scalars_[num] = value;
    scalarLabels_[num] = std::move(label);
  }
  void setVectorData(int num, std::vector<NumericType> &v, std::string label = "vectorData") {
    vectors_[num] = v;
    vectorLabels_[num] = std::move(label);
  }
  void setVectorData(int num, std::vector<NumericType> &&v, std::string label = "vectorData") {
    vectors_[num] = std::move(v);
    vectorLabels_[num] = std::move(label);
  }
  void setVectorData(int num, size_t size, NumericType value, std::string label = "vectorData") {
    vectors_[num].assign(size, value);
    vectorLabels_[num] = std::move(label);
  }
  void setVectorData(int num, NumericType value, std::string label = "vectorData") {
    vectors_[num].assign(vectors_[num].size(), value);
    vectorLabels_[num] = std::move(label);
  }
  void appendVectorData(int num, const std::vector<NumericType> &v) {
    vectors_[num].insert(vectors_[num].end(), v.begin(), v.end());
  }
  void resizeAllVectorData(size_t size, NumericType val = 0) {
    for (auto &v : vectors_) {
      v.clear();
      v.resize(size, val);
    }
  }
  void setVectorMergeType(const std::vector<TracingDataMergeEnum> &m) { vectorMerge_ = m; }
  void setVectorMergeType(int num, TracingDataMergeEnum m) { vectorMerge_[num] = m; }
  void setScalarMergeType(const std::vector<TracingDataMergeEnum> &m) { scalarMerge_ = m; }
  void setScalarMergeType(int num, TracingDataMergeEnum m) { scalarMerge_[num] = m; }

  [[nodiscard]] std::vector<NumericType> &getVectorData(int i) { return vectors_[i]; }
  [[nodiscard]] const std::vector<NumericType> &getVectorData(int i) const { return vectors_[i]; }
  [[nodiscard]] std::vector<NumericType> &getVectorData(const std::string &label) {
    return vectors_[getVectorDataIndex(label)];
  }
  [[nodiscard]] std::vector<std::vector<NumericType>> &getVectorData() { return vectors_; }
  [[nodiscard]] const std::vector<std::vector<NumericType>> &getVectorData() const { return vectors_; }
  [[nodiscard]] NumericType &getScalarData(int i) { return scalars_[i]; }
  [[nodiscard]] const NumericType &getScalarData(int i) const { return scalars_[i]; }
  [[nodiscard]] NumericType &getScalarData(const std::string &label) { return scalars_[getScalarDataIndex(label)]; }
  [[nodiscard]] std::vector<NumericType> &getScalarData() { return scalars_; }
  [[nodiscard]] const std::vector<NumericType> &getScalarData() const { return scalars_; }
  [[nodiscard]] std::string getVectorDataLabel(int i) const {
    return i < (int)vectorLabels_.size() ? vectorLabels_[i] : std::string();
  }
  [[nodiscard]] std::string getScalarDataLabel(int i) const {
    return i < (int)scalarLabels_.size() ? scalarLabels_[i] : std::string();
  }
  [[nodiscard]] int getVectorDataIndex(const std::string &label) const { return find(vectorLabels_, label, "vector"); }
  [[nodiscard]] int getScalarDataIndex(const std::string &label) const { return find(scalarLabels_, label, "scalar"); }
  [[nodiscard]] TracingDataMergeEnum getVectorMergeType(int num) const { return vectorMerge_[num]; }
  [[nodiscard]] TracingDataMergeEnum getScalarMergeType(int num) const { return scalarMerge_[num]; }
};

// ---- particles --------------------------------------------------------------------
// rayUtil.hpp:49-63.  The built-in particles log nothing.  A stateful run-time model with a log_data hook
// (viennaray_amd/csrc/vr_particles.hpp) fills the log on the device: Trace::apply() takes the shape from `data` as the
// caller sized it and ADDS the apply's sums to it (the reference merges its per-thread logs into the Trace's and never
// clears them, rayTraceKernel.hpp:75-82, 345).
template <class NumericType> struct DataLog {
  std::vector<std::vector<NumericType>> data;
  // element-wise sum of two logs (the shorter extent of each row counts)
  void merge(DataLog<NumericType> &pOther) {
    const std::size_t rows = std::min(data.size(), pOther.data.size());
    for (std::size_t r = 0; r < rows; ++r) {
      const std::size_t cols = std::min(data[r].size(), pOther.data[r].size());
      std::transform(data[r].begin(), data[r].begin() + cols, pOther.data[r].begin(), data[r].begin(), std::plus<NumericType>());
    }
  }
};

} // namespace viennaray

namespace rayInternal {
using namespace viennacore;
// rayUtil.hpp:266-283: Marsaglia's rejection method — a point of the unit disc (pairs from U(-1,1) until inside)
// lifted onto the sphere.  The reference's arithmetic: the squared radius and the lift factor in double, the
// coordinates narrowed back to NumericType.
template <typename NumericType> viennacore::Vec3D<NumericType> pickRandomPointOnUnitSphere(viennacore::RNG &rngState) {
  static thread_local std::uniform_real_distribution<NumericType> symmetric(NumericType(-1), NumericType(1));
  NumericType u = 0, v = 0;
  double radiusSq = 2.;
  while (radiusSq >= 1.) {
    u = symmetric(rngState);
    v = symmetric(rngState);
    radiusSq = u * u + v * v;
  }
  const double lift = 2. * std::sqrt(1. - radiusSq);
  u *= lift;
  v *= lift;
  const NumericType w = 1. - 2 * radiusSq;
  return viennacore::Vec3D<NumericType>{u, v, w};
}
// rayUtil.hpp:145-202: {rayDir, firstDir, secondDir, minMax, posNeg}
inline std::array<int, 5> getTraceSettings(unsigned sourceDir) {
  switch (sourceDir) {
  case 0: return {0, 1, 2, 1, -1}; // POS_X
  case 1: return {0, 1, 2, 0, 1};  // NEG_X
  case 2: return {1, 0, 2, 1, -1}; // POS_Y
  case 3: return {1, 0, 2, 0, 1};  // NEG_Y
  case 4: return {2, 0, 1, 1, -1}; // POS_Z
  default: return {2, 0, 1, 0, 1}; // NEG_Z
  }
}
template <int D> constexpr double DiskFactor = 0.5 * (D == 3 ? 1.7320508 : 1.41421356237) * (1 + 1e-5); // rayUtil.hpp:99-101

// rayUtil.hpp:104-143 (direction: viennaray::TraceDirection, passed as its underlying value 0..5)
template <typename NumericType, int D, class Direction>
void adjustBoundingBox(std::array<viennacore::Vec3D<NumericType>, 2> &bdBox, Direction const direction,
                       NumericType discRadius) {
  if constexpr (D == 2) {
    bdBox[0][2] -= discRadius;
    bdBox[1][2] += discRadius;
  }
  switch ((unsigned)direction) {
  case 0: bdBox[1][0] += 2 * discRadius; break;
  case 1: bdBox[0][0] -= 2 * discRadius; break;
  case 2: bdBox[1][1] += 2 * discRadius; break;
  case 3: bdBox[0][1] -= 2 * discRadius; break;
  case 4: bdBox[1][2] += 2 * discRadius; break;
  default: bdBox[0][2] -= 2 * discRadius; break;
  }
}
template <class Direction> std::array<int, 5> getTraceSettings(Direction d) { return getTraceSettings((unsigned)d); }

// rayUtil.hpp:564-611
// rayUtil.hpp:564-611: a regular lattice of ray origins on the source face of the bounding box, about `pNumPoints`
// of them, in the proportion of the face's sides; margins of 1e-4 keep the origins off the walls.  The lattice is
// walked by repeated addition like the reference's (the float sums ARE the coordinates: tests/createSourceGrid).
template <typename NumericType, int D>
[[nodiscard]] std::vector<viennacore::Vec3D<NumericType>>
createSourceGrid(const std::array<viennacore::Vec3D<NumericType>, 2> &pBdBox, const size_t pNumPoints,
                 const NumericType pGridDelta, const std::array<int, 5> &pTraceSettings) {
  const int axisRay = pTraceSettings[0], axisA = pTraceSettings[1], axisB = pTraceSettings[2];
  const int sourceSide = pTraceSettings[3];
  constexpr double margin = 1e-4;
  const auto sideA = pBdBox[1][axisA] - pBdBox[0][axisA];
  const auto sideB = pBdBox[1][axisB] - pBdBox[0][axisB];
  // lattice counts: first from the grid spacing (only their integer ratio survives), then from the requested total
  size_t countA = static_cast<size_t>(round(sideA / pGridDelta));
  size_t countB = static_cast<size_t>(round(sideB / pGridDelta));
  const unsigned long aspect = countA / countB;
  countA = static_cast<size_t>(std::sqrt(pNumPoints * aspect));
  countB = static_cast<size_t>(std::sqrt(pNumPoints / aspect));
  const auto stepA = (sideA - 2 * margin) / static_cast<NumericType>(countA - 1);
  const auto stepB = (sideB - 2 * margin) / static_cast<NumericType>(countB - 1);

  std::vector<viennacore::Vec3D<NumericType>> lattice;
  lattice.reserve(pNumPoints);
  viennacore::Vec3D<NumericType> origin;
  origin[axisRay] = pBdBox[sourceSide][axisRay];
  auto b = pBdBox[0][axisB] + margin;
  while (b <= pBdBox[1][axisB] - margin) {
    origin[axisB] = D == 2 ? decltype(b)(0) : b;
    auto a = pBdBox[0][axisA] + margin;
    while (a <= pBdBox[1][axisA] - margin) {
      origin[axisA] = a;
      lattice.push_back(origin);
      a += stepA;
    }
    b += stepB;
  }
  lattice.shrink_to_fit();
  return lattice;
}
} // namespace rayInternal

namespace viennaray {
using namespace viennacore;

// rayReflection.hpp:13-120 — the host-side reflection functions user particles call
template <typename NumericType, int D = 3>
[[nodiscard]] Vec3D<NumericType> ReflectionSpecular(const Vec3D<NumericType> &rayDir, const Vec3D<NumericType> &geomNormal) {
  auto dirOldInv = Inv(rayDir);
  return NumericType(2 * DotProduct(geomNormal, dirOldInv)) * geomNormal - dirOldInv;
}
// rayReflection.hpp:31-50: cosine-distributed about the normal = a uniform point of the unit sphere pushed along the
// normal and renormalised (2-D: the z component is dropped before the renormalisation)
template <typename NumericType, int D>
[[nodiscard]] Vec3D<NumericType> ReflectionDiffuse(const Vec3D<NumericType> &geomNormal, RNG &rngState) {
  Vec3D<NumericType> lobe = rayInternal::pickRandomPointOnUnitSphere<NumericType>(rngState);
  for (int axis = 0; axis < 2; ++axis)
    lobe[axis] += geomNormal[axis];
  lobe[2] = D == 3 ? NumericType(lobe[2] + geomNormal[2]) : NumericType(0);
  Normalize(lobe);
  return lobe;
}
// ReflectionConedCosine (rayReflection.hpp:52-120) assembled from two pieces of this library's own: the frame
// around the mirror direction and the accept-reject draw of the lobe's polar angle.  The arithmetic (types,
// operation order, engine outputs consumed) is the reference's — tests/aux/facade_units.cpp compares 10^5
// samples bit for bit with the oracle's restatement — the code is not.
namespace detail {
// two unit vectors completing `axis` (unit length) to a right-handed frame; the closed form has its pole at -z
template <typename NumericType> struct LobeFrame {
  Vec3D<NumericType> u, v;
  explicit LobeFrame(const Vec3D<NumericType> &axis) {
    const NumericType one(1);
    if (axis[2] < NumericType(-0.999999)) {
      u = Vec3D<NumericType>{NumericType(0), -one, NumericType(0)};
      v = Vec3D<NumericType>{-one, NumericType(0), NumericType(0)};
      return;
    }
    const NumericType k = one / (one + axis[2]);
    const NumericType mixed = -axis[0] * axis[1] * k;
    u = Vec3D<NumericType>{one - axis[0] * axis[0] * k, mixed, -axis[0]};
    v = Vec3D<NumericType>{mixed, one - axis[1] * axis[1] * k, -axis[1]};
  }
  // the direction with polar angle (sin, cos) = (sp, cp) and azimuth (sin, cos) = (sa, ca) about `axis`
  Vec3D<NumericType> at(const Vec3D<NumericType> &axis, NumericType sp, NumericType cp, NumericType sa, NumericType ca) const {
    Vec3D<NumericType> r;
    for (int k = 0; k < 3; ++k)
      r[k] = sp * (ca * u[k] + sa * v[k]) + cp * axis[k];
    return r;
  }
};
// polar angle of the cosine lobe squeezed into [0, cone]: proposals theta = cone * sqrt(1 - sqrt(U1)) are accepted
// when U2 * theta * sqrt(U1) <= cos(pi/2 * theta / cone) * sin(theta); two engine outputs per proposal
inline double lobePolarAngle(RNG &rng, double cone) {
  std::uniform_real_distribution<double> unit(0.0, 1.0);
  while (true) {
    const double rootU = std::sqrt(unit(rng));
    const double frac = std::sqrt(std::max(1.0 - rootU, 0.0));
    const double theta = cone * frac;
    const double bound = std::cos(M_PI_2 * frac) * std::sin(theta);
    if (unit(rng) * theta * rootU <= bound)
      return theta;
  }
}
} // namespace detail

template <typename NumericType, int D>
[[nodiscard]] Vec3D<NumericType> ReflectionConedCosine(const Vec3D<NumericType> &rayDir, const Vec3D<NumericType> &geomNormal,
                                                       RNG &rng, const NumericType maxConeAngle) {
  // the two ends of the family: a mirror, and the plain cosine lobe about the normal
  if (!(maxConeAngle > NumericType(0)))
    return ReflectionSpecular<NumericType>(rayDir, geomNormal);
  if (maxConeAngle >= M_PI_2)
    return ReflectionDiffuse<NumericType, D>(geomNormal, rng);
  Vec3D<NumericType> mirror = ReflectionSpecular<NumericType>(rayDir, geomNormal);
  Normalize(mirror);
  const detail::LobeFrame<NumericType> frame(mirror);
  const double theta = detail::lobePolarAngle(rng, maxConeAngle);
  const NumericType sinTheta = std::sin(theta), cosTheta = std::cos(theta);
  std::uniform_real_distribution<double> unit(0.0, 1.0);
  const double azimuth = 2.0 * M_PI * unit(rng);
  const NumericType sinAz = std::sin(azimuth), cosAz = std::cos(azimuth);
  Vec3D<NumericType> out = frame.at(mirror, sinTheta, cosTheta, sinAz, cosAz);
  // a sample below the surface is mirrored back above it
  if (const NumericType below = DotProduct(out, geomNormal); below <= NumericType(0))
    out = out - NumericType(NumericType(2) * below) * geomNormal;
  if constexpr (D == 2)
    out[2] = NumericType(0);
  Normalize(out);
  return out;
}

// raySource.hpp:10-19
template <typename NumericType> class Source {
public:
  virtual ~Source() = default;
  virtual std::array<Vec3D<NumericType>, 2> getOriginAndDirection(size_t idx, RNG &rngState) const = 0;
  [[nodiscard]] virtual size_t getNumPoints() const = 0;
  virtual NumericType getSourceArea() const = 0;
  virtual NumericType getInitialRayWeight(const size_t) const { return 1.; }
};

// SourceGrid (raySourceGrid.hpp:9-74): rays start at explicit grid points (origin = grid[idx mod n]) with a
// power-cosine direction about the tracing axis.  The tracer recognises the type and runs it in the generator
// kernel (vr_set_source_grid); this host version exists for user code that calls it directly and follows the
// reference's arithmetic (float cosf / sinf / sqrtf, two engine outputs per ray).
template <typename NumericType, int D> class SourceGrid : public Source<NumericType> {
  using boundingBoxType = std::array<Vec3D<NumericType>, 2>;

public:
  SourceGrid(const boundingBoxType &boundingBox, std::vector<Vec3D<NumericType>> &sourceGrid, NumericType cosinePower,
             const std::array<int, 5> &traceSettings)
      : box_(boundingBox), points_(sourceGrid), axis_{traceSettings[0], traceSettings[1], traceSettings[2]},
        sign_(static_cast<NumericType>(traceSettings[4])), exponent_(NumericType(2) / (cosinePower + NumericType(1))) {}

  std::array<Vec3D<NumericType>, 2> getOriginAndDirection(const size_t idx, RNG &rngState) const override {
    std::uniform_real_distribution<NumericType> unit;
    const NumericType azimuthDraw = unit(rngState);
    const NumericType polarDraw = unit(rngState);
    const NumericType cosSq = pow(polarDraw, exponent_); // cos^2 of the polar angle
    const float along = sqrtf(cosSq), across = sqrtf(1.f - cosSq);
    Vec3D<NumericType> d{NumericType(0), NumericType(0), NumericType(0)};
    d[axis_[0]] = sign_ * along;
    d[axis_[1]] = cosf(M_PI * 2.f * azimuthDraw) * across;
    if constexpr (D == 3)
      d[axis_[2]] = sinf(M_PI * 2.f * azimuthDraw) * across;
    Normalize(d);
    return {points_[idx % points_.size()], d};
  }
  [[nodiscard]] size_t getNumPoints() const override { return points_.size(); }
  // the face of the bounding box the rays start from
  NumericType getSourceArea() const override {
    NumericType area = box_[1][axis_[1]] - box_[0][axis_[1]];
    if constexpr (D == 3)
      area *= box_[1][axis_[2]] - box_[0][axis_[2]];
    return area;
  }
  [[nodiscard]] const std::vector<Vec3D<NumericType>> &getGrid() const { return points_; }

private:
  const boundingBoxType box_;
  const std::vector<Vec3D<NumericType>> &points_;
  const std::array<int, 3> axis_; // tracing axis, first and second transverse axis
  const NumericType sign_;        // rays travel towards -/+ the tracing axis
  const NumericType exponent_;
};

#define VIENNARAY_PARTICLE_STOP                                                                                         \
  std::pair<NumericType, Vec3D<NumericType>> { NumericType(1), Vec3D<NumericType>{} }

// rayParticle.hpp:21-81
template <typename NumericType> class AbstractParticle {
public:
  virtual ~AbstractParticle() = default;
  virtual std::unique_ptr<AbstractParticle> clone() const = 0;
  virtual void initNew(RNG &rngState) = 0;
  virtual Vec3D<NumericType> initNewWithDirection(RNG &rngState) = 0;
  virtual std::pair<NumericType, Vec3D<NumericType>>
  surfaceReflection(NumericType rayWeight, const Vec3D<NumericType> &rayDir, const Vec3D<NumericType> &geomNormal,
                    const unsigned int primId, const int materialId, const TracingData<NumericType> *globalData,
                    RNG &rngState) = 0;
  virtual void surfaceCollision(NumericType rayWeight, const Vec3D<NumericType> &rayDir,
                                const Vec3D<NumericType> &geomNormal, const unsigned int primID, const int materialId,
                                TracingData<NumericType> &localData, const TracingData<NumericType> *globalData,
                                RNG &rngState) = 0;
  virtual NumericType getSourceDistributionPower() const = 0;
  virtual NumericType getMeanFreePath() const = 0;
  [[nodiscard]] virtual std::vector<std::string> getLocalDataLabels() const = 0;
  virtual void logData(DataLog<NumericType> &log) = 0;

  /// NOT in the reference: how this particle runs on the device.  Fill `pod` with a model of the
  /// device registry (viennaray_amd/csrc/vr_particles.hpp) and return true.  The default (false)
  /// means the particle exists only as host virtuals, which a HIP kernel cannot call.
  virtual bool deviceModel(vr_particle &pod) const {
    (void)pod;
    return false;
  }
};

// rayParticle.hpp:83-122: CRTP base implementing clone() and the no-op defaults
template <typename Derived, typename NumericType> class Particle : public AbstractParticle<NumericType> {
public:
  std::unique_ptr<AbstractParticle<NumericType>> clone() const final {
    return std::make_unique<Derived>(static_cast<Derived const &>(*this));
  }
  void initNew(RNG &) override {}
  Vec3D<NumericType> initNewWithDirection(RNG &) override { return Vec3D<NumericType>{0, 0, 0}; }
  std::pair<NumericType, Vec3D<NumericType>> surfaceReflection(NumericType, const Vec3D<NumericType> &,
                                                               const Vec3D<NumericType> &, const unsigned int, const int,
                                                               const TracingData<NumericType> *, RNG &) override {
    return VIENNARAY_PARTICLE_STOP;
  }
  void surfaceCollision(NumericType, const Vec3D<NumericType> &, const Vec3D<NumericType> &, const unsigned int, const int,
                        TracingData<NumericType> &, const TracingData<NumericType> *, RNG &) override {}
  NumericType getSourceDistributionPower() const override { return 1.; }
  NumericType getMeanFreePath() const override { return -1.; }
  [[nodiscard]] std::vector<std::string> getLocalDataLabels() const override { return {}; }
  void logData(DataLog<NumericType> &) override {}

protected:
  Particle() = default;
  Particle(const Particle &) = default;
  Particle(Particle &&) = default;
};

// rayParticle.hpp:126-163
template <typename NumericType, int D>
class DiffuseParticle : public Particle<DiffuseParticle<NumericType, D>, NumericType> {
  const NumericType stickingProbability_;
  const std::string dataLabel_;

public:
  DiffuseParticle(NumericType stickingProbability, std::string dataLabel)
      : stickingProbability_(stickingProbability), dataLabel_(std::move(dataLabel)) {}
  std::pair<NumericType, Vec3D<NumericType>> surfaceReflection(NumericType, const Vec3D<NumericType> &,
                                                               const Vec3D<NumericType> &geomNormal, const unsigned int,
                                                               const int, const TracingData<NumericType> *,
                                                               RNG &rngState) final {
    return {stickingProbability_, ReflectionDiffuse<NumericType, D>(geomNormal, rngState)};
  }
  void surfaceCollision(NumericType rayWeight, const Vec3D<NumericType> &, const Vec3D<NumericType> &,
                        const unsigned int primID, const int, TracingData<NumericType> &localData,
                        const TracingData<NumericType> *, RNG &) final {
    localData.getVectorData(0)[primID] += rayWeight;
  }
  NumericType getSourceDistributionPower() const final { return 1.; }
  [[nodiscard]] std::vector<std::string> getLocalDataLabels() const final { return {dataLabel_}; }
  bool deviceModel(vr_particle &pod) const final {
    pod = vr_particle{VR_PARTICLE_DIFFUSE, (float)stickingProbability_, 1.f, 0, nullptr, nullptr, 0.f, -1.f};
    return true;
  }
};

// rayParticle.hpp:165-204
template <typename NumericType, int D>
class SpecularParticle : public Particle<SpecularParticle<NumericType, D>, NumericType> {
  const NumericType stickingProbability_;
  const NumericType sourcePower_;
  const std::string dataLabel_;

public:
  SpecularParticle(NumericType stickingProbability, NumericType sourcePower, std::string dataLabel)
      : stickingProbability_(stickingProbability), sourcePower_(sourcePower), dataLabel_(std::move(dataLabel)) {}
  std::pair<NumericType, Vec3D<NumericType>> surfaceReflection(NumericType, const Vec3D<NumericType> &rayDir,
                                                               const Vec3D<NumericType> &geomNormal, const unsigned int,
                                                               const int, const TracingData<NumericType> *, RNG &) final {
    return {stickingProbability_, ReflectionSpecular<NumericType, D>(rayDir, geomNormal)};
  }
  void surfaceCollision(NumericType rayWeight, const Vec3D<NumericType> &, const Vec3D<NumericType> &,
                        const unsigned int primID, const int, TracingData<NumericType> &localData,
                        const TracingData<NumericType> *, RNG &) final {
    localData.getVectorData(0)[primID] += rayWeight;
  }
  NumericType getSourceDistributionPower() const final { return sourcePower_; }
  [[nodiscard]] std::vector<std::string> getLocalDataLabels() const final { return {dataLabel_}; }
  bool deviceModel(vr_particle &pod) const final {
    pod = vr_particle{VR_PARTICLE_SPECULAR, (float)stickingProbability_, (float)sourcePower_, 0, nullptr, nullptr, 0.f, -1.f};
    return true;
  }
};

// ---- plug-in particles of the device registry (NOT in the reference's rayParticle.hpp; written
//      against AbstractParticle the way a ViennaPS model is, with a device model each) ------------
// sticking + ReflectionConedCosine(maxConeAngle), optional mean free path; collects like SpecularParticle
template <typename NumericType, int D>
class ConedCosineParticle : public Particle<ConedCosineParticle<NumericType, D>, NumericType> {
  const NumericType stickingProbability_, sourcePower_, coneAngle_, meanFreePath_;
  const std::string dataLabel_;

public:
  ConedCosineParticle(NumericType stickingProbability, NumericType sourcePower, NumericType maxConeAngle,
                      std::string dataLabel, NumericType meanFreePath = NumericType(-1))
      : stickingProbability_(stickingProbability), sourcePower_(sourcePower), coneAngle_(maxConeAngle),
        meanFreePath_(meanFreePath), dataLabel_(std::move(dataLabel)) {}
  std::pair<NumericType, Vec3D<NumericType>> surfaceReflection(NumericType, const Vec3D<NumericType> &rayDir,
                                                               const Vec3D<NumericType> &geomNormal, const unsigned int,
                                                               const int, const TracingData<NumericType> *,
                                                               RNG &rngState) final {
    return {stickingProbability_, ReflectionConedCosine<NumericType, D>(rayDir, geomNormal, rngState, coneAngle_)};
  }
  void surfaceCollision(NumericType rayWeight, const Vec3D<NumericType> &, const Vec3D<NumericType> &,
                        const unsigned int primID, const int, TracingData<NumericType> &localData,
                        const TracingData<NumericType> *, RNG &) final {
    localData.getVectorData(0)[primID] += rayWeight;
  }
  NumericType getSourceDistributionPower() const final { return sourcePower_; }
  NumericType getMeanFreePath() const final { return meanFreePath_; }
  [[nodiscard]] std::vector<std::string> getLocalDataLabels() const final { return {dataLabel_}; }
  bool deviceModel(vr_particle &pod) const final {
    pod = vr_particle{VR_PARTICLE_CONED_COSINE, (float)stickingProbability_, (float)sourcePower_, 0, nullptr, nullptr,
                      (float)coneAngle_, (float)meanFreePath_};
    return true;
  }
};

// a DiffuseParticle with two data labels: label 0 += w, label 1 += w * max(0, -d.n)
template <typename NumericType, int D>
class DiffuseCosineParticle : public Particle<DiffuseCosineParticle<NumericType, D>, NumericType> {
  const NumericType stickingProbability_;
  const std::string dataLabel_, cosineLabel_;

public:
  DiffuseCosineParticle(NumericType stickingProbability, std::string dataLabel, std::string cosineLabel)
      : stickingProbability_(stickingProbability), dataLabel_(std::move(dataLabel)), cosineLabel_(std::move(cosineLabel)) {}
  std::pair<NumericType, Vec3D<NumericType>> surfaceReflection(NumericType, const Vec3D<NumericType> &,
                                                               const Vec3D<NumericType> &geomNormal, const unsigned int,
                                                               const int, const TracingData<NumericType> *,
                                                               RNG &rngState) final {
    return {stickingProbability_, ReflectionDiffuse<NumericType, D>(geomNormal, rngState)};
  }
  void surfaceCollision(NumericType rayWeight, const Vec3D<NumericType> &rayDir, const Vec3D<NumericType> &geomNormal,
                        const unsigned int primID, const int, TracingData<NumericType> &localData,
                        const TracingData<NumericType> *, RNG &) final {
    localData.getVectorData(0)[primID] += rayWeight;
    localData.getVectorData(1)[primID] += rayWeight * std::max(-DotProduct(rayDir, geomNormal), NumericType(0));
  }
  NumericType getSourceDistributionPower() const final { return 1.; }
  [[nodiscard]] std::vector<std::string> getLocalDataLabels() const final { return {dataLabel_, cosineLabel_}; }
  bool deviceModel(vr_particle &pod) const final {
    pod = vr_particle{VR_PARTICLE_DIFFUSE_COSINE, (float)stickingProbability_, 1.f, 0, nullptr, nullptr, 0.f, -1.f};
    return true;
  }
};

// The pattern `globalData` exists for (ViennaPS surface models): a diffuse particle whose sticking falls with the coverage
// of the primitive it meets.  coverage = vector `coverageVector` of the TracingData given to Trace::setGlobalData.
template <typename NumericType, int D>
class CoverageStickingParticle : public Particle<CoverageStickingParticle<NumericType, D>, NumericType> {
  const NumericType stickingProbability_;
  const std::string dataLabel_;
  const int coverageVector_;

public:
  CoverageStickingParticle(NumericType stickingProbability, std::string dataLabel, int coverageVector = 0)
      : stickingProbability_(stickingProbability), dataLabel_(std::move(dataLabel)), coverageVector_(coverageVector) {}
  std::pair<NumericType, Vec3D<NumericType>> surfaceReflection(NumericType, const Vec3D<NumericType> &,
                                                               const Vec3D<NumericType> &geomNormal,
                                                               const unsigned int primID, const int,
                                                               const TracingData<NumericType> *globalData,
                                                               RNG &rngState) final {
    NumericType coverage = 0;
    if (globalData && coverageVector_ < (int)globalData->getVectorData().size() &&
        primID < globalData->getVectorData(coverageVector_).size())
      coverage = globalData->getVectorData(coverageVector_)[primID];
    return {stickingProbability_ * (NumericType(1) - coverage), ReflectionDiffuse<NumericType, D>(geomNormal, rngState)};
  }
  void surfaceCollision(NumericType rayWeight, const Vec3D<NumericType> &, const Vec3D<NumericType> &,
                        const unsigned int primID, const int, TracingData<NumericType> &localData,
                        const TracingData<NumericType> *, RNG &) final {
    localData.getVectorData(0)[primID] += rayWeight;
  }
  NumericType getSourceDistributionPower() const final { return 1.; }
  [[nodiscard]] std::vector<std::string> getLocalDataLabels() const final { return {dataLabel_}; }
  bool deviceModel(vr_particle &pod) const final {
    pod = vr_particle{VR_PARTICLE_COVERAGE_STICKING, (float)stickingProbability_, 1.f, 0, nullptr, nullptr, 0.f, -1.f, {}};
    pod.params[0] = (float)coverageVector_;
    return true;
  }
};

// A particle whose device model was registered at run time (Trace::registerParticleModel — the counterpart of the
// reference's GPU path naming user callables per particle, gpu/raygCallableConfig.hpp:7-18): `kind` is what the
// registration returned, `params` go to the model as ModelCtx::params.  The host virtuals keep the no-op defaults of
// Particle<>: the per-hit logic IS the device model.
template <typename NumericType, int D>
class UserModelParticle : public Particle<UserModelParticle<NumericType, D>, NumericType> {
  const int kind_;
  const NumericType stickingProbability_, sourcePower_;
  const std::vector<std::string> dataLabels_;
  std::array<float, 8> params_{};

public:
  UserModelParticle(int kind, NumericType stickingProbability, std::vector<std::string> dataLabels,
                    NumericType sourcePower = NumericType(1), const std::vector<float> &params = {})
      : kind_(kind), stickingProbability_(stickingProbability), sourcePower_(sourcePower), dataLabels_(std::move(dataLabels)) {
    for (size_t k = 0; k < params.size() && k < params_.size(); ++k)
      params_[k] = params[k];
  }
  NumericType getSourceDistributionPower() const final { return sourcePower_; }
  [[nodiscard]] std::vector<std::string> getLocalDataLabels() const final { return dataLabels_; }
  bool deviceModel(vr_particle &pod) const final {
    pod = vr_particle{kind_, (float)stickingProbability_, (float)sourcePower_, 0, nullptr, nullptr, 0.f, -1.f, {}};
    for (size_t k = 0; k < params_.size(); ++k)
      pod.params[k] = params_[k];
    return true;
  }
};

/// what Trace::castRays returns, one entry per ray (not in the reference; vr_cast_rays, whose header comment has the
/// definition): primIDs >= 0 the primitive hit, VR_CAST_MISS (-1) or VR_CAST_WALL (-2); distances +inf and hitPoints NaN
/// for a miss; boundaryHits the walls the ray was continued at
template <class NumericType> struct CastResult {
  std::vector<int> primIDs;
  std::vector<NumericType> distances;
  std::vector<Vec3D<NumericType>> hitPoints;
  std::vector<unsigned> boundaryHits;
};

/// how Trace::gatherFlux samples (VR_GATHER_*): NORMAL the cosine law about the primitive's normal, SOURCE the source's
/// power-cosine law about the direction to the source plane (cosinePower >= 2, no emission)
enum class GatherMode : unsigned { NORMAL = VR_GATHER_NORMAL, SOURCE = VR_GATHER_SOURCE };
/// what a vertex of Trace::gatherPaths does (VR_GATHER_REFLECT_*): SPECULAR the mirror direction, DIFFUSE the cosine law
/// about the normal hit
enum class GatherReflection : unsigned { SPECULAR = VR_GATHER_REFLECT_SPECULAR, DIFFUSE = VR_GATHER_REFLECT_DIFFUSE };

// ---- Trace<T,D> ----------------------------------------------------------------------
template <class NumericType, int D> class Trace {
public:
  Trace() {
    if (vr_create(&ctx_, 0) != VR_OK) {
      ctx_ = nullptr;
      RTInfo_.error = true;
      std::cerr << "viennaray_amd: no usable HIP device (there is no CPU fallback)\n";
    }
  }
  Trace(const Trace &) = delete;
  Trace &operator=(const Trace &) = delete;
  Trace(Trace &&) = delete;
  Trace &operator=(Trace &&) = delete;
  virtual ~Trace() { vr_destroy(ctx_); }

  /// Run the ray tracer
  virtual void apply() {
    if (!ctx_ || pParticle_ == nullptr) {
      RTInfo_.error = true;
      std::cerr << "No particle was specified in rayTrace. Aborting.\n";
      return;
    }
    if (!particleOnDevice_) {
      RTInfo_.error = true;
      std::cerr << "viennaray_amd: this particle type has no device model (AbstractParticle::deviceModel): its "
                   "surfaceCollision / surfaceReflection exist only as host virtuals, which a HIP kernel cannot call. "
                   "Add a model to viennaray_amd/csrc/vr_particles.hpp and override deviceModel().\n";
      return;
    }
    if (setterError_) { // a setter was refused (e.g. too many primitives): do not trace something else
      RTInfo_.error = true;
      std::cerr << vr_last_error(ctx_) << "\n";
      return;
    }
    if (pSource_ && !sourceOnDevice_ && !uploadHostSource())
      return;
    uploadGlobalData();
    const bool logging = setDataLogShape();
    const int rc = world_ > 1 ? vr_apply_sharded(ctx_, rank_, world_, reduce_, reduceUser_) : vr_apply(ctx_);
    vr_trace_info i{};
    vr_get_trace_info(ctx_, &i);
    RTInfo_.numRays = i.numRays;
    RTInfo_.totalRaysTraced = i.totalRaysTraced;
    RTInfo_.nonGeometryHits = i.nonGeometryHits;
    RTInfo_.geometryHits = i.geometryHits;
    RTInfo_.particleHits = i.particleHits;
    RTInfo_.boundaryHits = i.boundaryHits;
    RTInfo_.reflections = i.reflections;
    RTInfo_.time = i.time;
    // NumericType = double (rayTrace.hpp:15 allows it): positions, directions and weights are narrowed to float at the
    // C ABI and traced in float — the result is NumericType = float's.  Narrower arithmetic than asked for: flagged.
    RTInfo_.warning = i.warning != 0 || !std::is_same_v<NumericType, float>;
    if constexpr (!std::is_same_v<NumericType, float>) {
      static bool told = false;
      if (!told) {
        told = true;
        std::cerr << "viennaray_amd: NumericType is not float: geometry and results are narrowed to float at the device "
                     "boundary (TraceInfo.warning is set).\n";
      }
    }
    RTInfo_.error = i.error != 0 || rc != VR_OK;
    if (rc != VR_OK) {
      std::cerr << vr_last_error(ctx_) << "\n";
      return;
    }
    if (logging)
      mergeDataLog();
    // rayTraceDisk.hpp:40-47: one vector per data label of the particle (of every particle of a list, in order)
    auto labels = pParticle_->getLocalDataLabels();
    for (const auto &extra : moreParticles_) {
      auto l = extra->getLocalDataLabels();
      labels.insert(labels.end(), l.begin(), l.end());
    }
    localData_.setNumberOfVectorData((int)labels.size());
    const uint32_t n = vr_num_primitives(ctx_);
    const uint32_t nd = vr_num_data(ctx_);
    for (int k = 0; k < (int)labels.size(); ++k) {
      localData_.setVectorData(k, n, NumericType(0), labels[k]);
      if ((uint32_t)k >= nd)
        continue;
      if constexpr (std::is_same_v<NumericType, float>) {
        vr_get_flux_data(ctx_, (uint32_t)k, localData_.getVectorData(k).data(), n);
      } else {
        std::vector<float> tmp(n);
        vr_get_flux_data(ctx_, (uint32_t)k, tmp.data(), n);
        for (uint32_t j = 0; j < n; ++j)
          localData_.getVectorData(k)[j] = (NumericType)tmp[j];
      }
    }
  }

  template <typename ParticleType,
            std::enable_if_t<std::is_base_of_v<AbstractParticle<NumericType>, ParticleType>, bool> = true>
  void setParticleType(std::unique_ptr<ParticleType> const &particle) {
    pParticle_ = particle->clone();
    moreParticles_.clear();
    vr_particle pod{};
    particleOnDevice_ = pParticle_->deviceModel(pod);
    particleKinds_.assign(1, pod.kind);
    if (ctx_ && particleOnDevice_)
      check(vr_set_particle(ctx_, &pod));
  }
  /// NOT in the reference's CPU Trace: compile a device particle model at run time (vr_register_particle_model: HIP source
  /// of `struct VrUserModel`, see viennaray_amd/csrc/vr_particles.hpp) and get the kind id for a UserModelParticle.
  /// Returns -1 (and sets TraceInfo.error) if the model does not compile.
  int registerParticleModel(const std::string &name, const std::string &source, int numData = 1, bool needsFull = false) {
    int32_t kind = -1;
    if (ctx_)
      check(vr_register_particle_model(ctx_, name.c_str(), source.c_str(), numData, needsFull ? VR_MODEL_NEEDS_FULL : 0, &kind));
    return kind;
  }
  /// ... a model with per-ray state: numState = VrUserModel::kStateWords (1 .. 4; init / surface_reflection / collide
  /// hooks, vr_register_particle_model_ex; implies needsFull).  SourceRandom only.
  int registerParticleModel(const std::string &name, const std::string &source, int numData, int numState) {
    int32_t kind = -1;
    if (ctx_)
      check(vr_register_particle_model_ex(ctx_, name.c_str(), source.c_str(), numData, numState, 0, &kind));
    return kind;
  }
  /// NOT in the reference's CPU Trace (its gpu::Trace keeps a particle list, gpu/raygTrace.hpp:163-248): several
  /// particles traced in ONE apply() — the same seed for all, one generator pass per source distribution;
  /// getLocalData() holds particle 0's data labels, then particle 1's, ...; getRayTraceInfo() their summed counters.
  void setParticleTypes(const std::vector<std::unique_ptr<AbstractParticle<NumericType>>> &particles) {
    if (particles.empty())
      return;
    std::vector<vr_particle> pods(particles.size());
    moreParticles_.clear();
    particleOnDevice_ = true;
    for (size_t q = 0; q < particles.size(); ++q) {
      auto copy = particles[q]->clone();
      particleOnDevice_ = copy->deviceModel(pods[q]) && particleOnDevice_;
      if (q == 0)
        pParticle_ = std::move(copy);
      else
        moreParticles_.push_back(std::move(copy));
    }
    particleKinds_.clear();
    for (const vr_particle &pod : pods)
      particleKinds_.push_back(pod.kind);
    if (ctx_ && particleOnDevice_)
      check(vr_set_particles(ctx_, pods.data(), (uint32_t)pods.size()));
  }

  void setBoundaryConditions(BoundaryCondition boundaryConditions[D]) {
    int32_t b[3] = {0, 0, 0};
    for (int i = 0; i < D; ++i)
      b[i] = (int32_t)boundaryConditions[i];
    if (ctx_)
      check(vr_set_boundary_conditions(ctx_, b, D));
  }
  void setNumberOfRaysPerPoint(const size_t n) {
    numRaysPerPoint_ = n;
    numRaysFixed_ = 0;
    if (ctx_)
      check(vr_set_number_of_rays_per_point(ctx_, n));
  }
  void setNumberOfRaysFixed(const size_t n) {
    numRaysFixed_ = n;
    numRaysPerPoint_ = 0;
    if (ctx_)
      check(vr_set_number_of_rays_fixed(ctx_, n));
  }
  void setMaxReflections(const unsigned n) {
    if (ctx_)
      check(vr_set_max_reflections(ctx_, n));
  }
  void setMaxBoundaryHits(const unsigned n) {
    if (ctx_)
      check(vr_set_max_boundary_hits(ctx_, n));
  }
  void setSourceDirection(const TraceDirection direction) {
    if (ctx_)
      check(vr_set_source_direction(ctx_, (int)direction));
  }
  void setPrimaryDirection(const Vec3D<NumericType> primaryDirection) {
    const float d[3] = {(float)primaryDirection[0], (float)primaryDirection[1], (float)primaryDirection[2]};
    if (ctx_)
      check(vr_set_primary_direction(ctx_, d));
  }
  void setUseRandomSeeds(const bool useRand) {
    useRandomSeeds_ = useRand;
    if (ctx_)
      check(vr_set_use_random_seeds(ctx_, useRand ? 1 : 0));
  }
  void setRngSeed(const unsigned int seed) {
    rngSeed_ = seed;
    useRandomSeeds_ = false;
    if (ctx_)
      check(vr_set_rng_seed(ctx_, seed));
  }
  /// NOT in the reference: make apply() one rank of a multi-GPU trace (one process per GPU).  This rank
  /// traces its share of the global ray indices and `reduce` sums the int64 accumulators over the ranks
  /// (vr_rccl_allreduce of viennaray_amd_rccl.h = RCCL over xGMI); every rank ends with the full flux.
  void setDistributed(int rank, int world, vr_allreduce_fn reduce, void *user) {
    rank_ = rank;
    world_ = world;
    reduce_ = reduce;
    reduceUser_ = user;
  }
  /// VIENNARAY_USE_WDIST (a compile-time option of the reference, CMakeLists.txt:15) as a run-time switch
  void setUseWdist(const bool on) {
    if (ctx_)
      check(vr_set_use_wdist(ctx_, on ? 1 : 0));
  }
  // rayTrace.hpp:53-61.  SourceGrid goes to the generator kernel; any other Source is evaluated on the
  // host at apply() (uploadHostSource)
  void setSource(std::shared_ptr<Source<NumericType>> source) {
    pSource_ = std::move(source);
    sourceOnDevice_ = false;
    if (!ctx_ || !pSource_)
      return;
    if (auto *g = dynamic_cast<SourceGrid<NumericType, D> *>(pSource_.get())) {
      auto pts = flatten3(g->getGrid());
      check(vr_set_source_grid(ctx_, pts.data(), (uint32_t)g->getGrid().size()));
      check(vr_set_source_area(ctx_, (float)g->getSourceArea()));
      sourceOnDevice_ = true;
    }
  }
  void resetSource() {
    pSource_.reset();
    sourceOnDevice_ = false;
    if (ctx_)
      check(vr_set_source_grid(ctx_, nullptr, 0)); // also drops host rays
    if (ctx_)
      check(vr_set_source_area(ctx_, 0.f));
  }
  /// gpu/raygTrace.hpp:267-297: the rays of the next applies start ON the given points (numRaysFixed if set, else
  /// numRaysPerPoint, rays per point), leave along a cosine distribution about each point's normal from position +
  /// unit normal * sourceOffset and carry the point's weight; sampled on the device.  normalizeFlux(SOURCE) then uses
  /// sourceArea.  Takes the place of any other source; an empty set of points is clearSurfaceSource().
  void setSurfaceSource(const std::vector<Vec3D<NumericType>> &positions, const std::vector<Vec3D<NumericType>> &normals,
                        const std::vector<NumericType> &weights, NumericType sourceArea, NumericType sourceOffset) {
    if (!ctx_)
      return;
    if (positions.size() != normals.size() || positions.size() != weights.size() || positions.size() > 0xFFFFFFFFull) {
      setterError_ = true;
      RTInfo_.error = true;
      std::cerr << "viennaray_amd: setSurfaceSource: one normal and one weight per position.\n";
      return;
    }
    const auto pos = flatten3(positions), nrm = flatten3(normals);
    const std::vector<float> w(weights.begin(), weights.end());
    const int rc = vr_set_surface_source(ctx_, pos.data(), nrm.data(), w.data(), (uint32_t)positions.size(),
                                         (float)sourceArea, (float)sourceOffset);
    check(rc);
    if (rc == VR_OK && !positions.empty()) { // (a refused source leaves the previous one in place)
      pSource_.reset();
      sourceOnDevice_ = false;
    }
  }
  void clearSurfaceSource() {
    if (ctx_)
      check(vr_set_surface_source(ctx_, nullptr, nullptr, nullptr, 0, 0.f, 0.f));
  }
  /// NOT in the reference's CPU Trace: a user Source as DEVICE code (vr_register_source_model: HIP text of `struct
  /// VrUserSource`, see include/viennaray_amd.h), compiled into the ray generator.  Returns the id setSourceModel takes,
  /// -1 (and sets TraceInfo.error) if the text does not compile.  hasWeight = the text's kHasWeight.
  int registerSourceModel(const std::string &name, const std::string &source, bool hasWeight = false) {
    int32_t id = -1;
    if (ctx_ && vr_register_source_model(ctx_, name.c_str(), source.c_str(), hasWeight ? VR_SOURCE_HAS_WEIGHT : 0, &id) != VR_OK) {
      RTInfo_.error = true; // (nothing was set: the source in force stays, and later applies run)
      std::cerr << "viennaray_amd: " << vr_last_error(ctx_) << "\n";
      id = -1;
    }
    return id;
  }
  /// The rays of the next applies are sampled on the device by source model `id` (registerSourceModel; < 0: back to
  /// SourceRandom) with up to 16 params and one table; numRays == 0 keeps the ray count of setNumberOfRaysPerPoint /
  /// setNumberOfRaysFixed, > 0 is the source's own.  Takes the place of any other source — setSource(std::shared_ptr<Source>)
  /// stays the host path — and a refusal leaves the previous one in place.
  void setSourceModel(int id, const std::vector<float> &params = {}, const std::vector<float> &table = {}, size_t numRays = 0) {
    if (!ctx_)
      return;
    const int rc = vr_set_source_model(ctx_, id, params.data(), (uint32_t)std::min<size_t>(params.size(), 0xFFFFFFFFull),
                                       table.data(), (uint32_t)std::min<size_t>(table.size(), 0xFFFFFFFFull), numRays);
    check(rc);
    if (rc == VR_OK && id >= 0) {
      pSource_.reset();
      sourceOnDevice_ = false;
    }
  }
  /// setSurfaceSource for tables that live on the device (vr_set_surface_source_device): dPositions / dNormals are
  /// DEVICE pointers to n rows of `ld` floats (2 or 3; 2 only for D == 2), dWeights to n floats, produced on `stream`
  /// (the caller's hipStream_t, nullptr = the null stream).  Packed and validated on the device; a refusal names the row
  /// as the host setter would and leaves the previous source in place.  The buffers are free again on return.
  void setSurfaceSourceDevice(const float *dPositions, const float *dNormals, const float *dWeights, size_t n, unsigned ld,
                              NumericType sourceArea, NumericType sourceOffset, void *stream = nullptr) {
    if (deviceCall(false, vr_set_surface_source_device, dPositions, dNormals, dWeights, n, ld, sourceArea, sourceOffset,
                   stream) &&
        n) {
      pSource_.reset();
      sourceOnDevice_ = false;
    }
  }
  /// setMaterialIds for ids that live on the device (vr_set_material_ids_device): n int32 in the caller's primitive
  /// order, produced on `stream`; a primitive beyond n has id 0.
  void setMaterialIdsDevice(const int32_t *dIds, size_t n, void *stream = nullptr) {
    deviceCall(false, vr_set_material_ids_device, dIds, n, stream);
  }
  void enableProgressBar() {}
  void disableProgressBar() {}

  virtual void normalizeFlux(std::vector<NumericType> &flux, NormalizationType norm = NormalizationType::SOURCE) {
    inPlace(flux, [&](float *p, uint32_t n) { return vr_normalize_flux(ctx_, p, n, (int)norm); });
  }
  virtual void smoothFlux(std::vector<NumericType> &flux, int numNeighbors = 1) {
    inPlace(flux, [&](float *p, uint32_t n) { return vr_smooth_flux(ctx_, p, n, numNeighbors); });
  }

  /// The flux of data label `dataIdx` written to DEVICE memory `dOut` (float32, one per primitive, caller's order):
  /// getLocalData().getVectorData(dataIdx) -> normalizeFlux(norm) -> smoothFlux(numNeighbors; 0 = none), computed and
  /// left on the device (vr_get_flux_device).  `stream`: the caller's hipStream_t (nullptr = the null stream), which is
  /// made to wait for the result; without smoothing nothing synchronises with the host.  false if it was refused.
  bool getFluxDevice(float *dOut, int dataIdx, NormalizationType norm, int numNeighbors, void *stream = nullptr) {
    return fluxDevice(dOut, dataIdx, (int)norm, numNeighbors, stream);
  }
  /// ... the raw flux, neither normalised nor smoothed
  bool getFluxDevice(float *dOut, int dataIdx = 0, void *stream = nullptr) {
    return fluxDevice(dOut, dataIdx, VR_NORM_NONE, 0, stream);
  }

  // ---- per-primitive values at the caller's points (not in the reference; vr_map_to_points*, whose header comment
  //      has the definition): the mean of the values over the primitive centres within `radius`, weighted by
  //      (1 - d / radius) * max(0, n_j . normal_i) — no gate without normals — or the nearest centre's value where that
  //      sum of weights is not positive.  Plain Euclidean distances; a 2-D scene ignores z.  Needs the scene build of the
  //      geometry in force: apply() first.
  /// dValues (one float per primitive, caller's order), dPoints / dNormals (m rows of ld = 2 or 3 floats, 2 only with
  /// D == 2; dNormals may be nullptr) and dOut (m floats) are DEVICE memory; getFluxDevice's stream rules.  false if it
  /// was refused.
  bool mapToPointsDevice(const float *dValues, const float *dPoints, const float *dNormals, size_t m, unsigned ld,
                         float radius, float *dOut, void *stream = nullptr) {
    return ctx_ && reported(vr_map_to_points_device(ctx_, dValues, vr_num_primitives(ctx_), dPoints, dNormals, (uint32_t)m,
                                                    ld, radius, dOut, stream));
  }
  /// getFluxDevice(dataIdx, norm, numNeighbors) mapped to the points, the flux never leaving the device
  bool getFluxAtPointsDevice(const float *dPoints, const float *dNormals, size_t m, unsigned ld, float radius, float *dOut,
                             int dataIdx, NormalizationType norm, int numNeighbors, void *stream = nullptr) {
    return ctx_ && reported(vr_get_flux_at_points_device(ctx_, (uint32_t)dataIdx, (int)norm, numNeighbors, dPoints, dNormals,
                                                         (uint32_t)m, ld, radius, dOut, stream));
  }
  /// ... the raw flux, neither normalised nor smoothed
  bool getFluxAtPointsDevice(const float *dPoints, const float *dNormals, size_t m, unsigned ld, float radius, float *dOut,
                             int dataIdx = 0, void *stream = nullptr) {
    return ctx_ && reported(vr_get_flux_at_points_device(ctx_, (uint32_t)dataIdx, VR_NORM_NONE, 0, dPoints, dNormals,
                                                         (uint32_t)m, ld, radius, dOut, stream));
  }
  /// the host form: `values` per primitive, `points` (and `normals`, empty = no gate) as rows of three; the mapped
  /// values, empty (with the library's message on std::cerr) if it was refused
  [[nodiscard]] std::vector<NumericType> mapToPoints(const std::vector<NumericType> &values,
                                                     const std::vector<std::array<NumericType, 3>> &points,
                                                     const std::vector<std::array<NumericType, 3>> &normals, float radius) {
    const std::vector<float> v(values.begin(), values.end());
    std::vector<float> p(3 * points.size()), q(3 * normals.size()), raw(points.size());
    for (size_t i = 0; i < points.size(); ++i)
      for (int k = 0; k < 3; ++k)
        p[3 * i + k] = (float)points[i][k];
    for (size_t i = 0; i < normals.size(); ++i)
      for (int k = 0; k < 3; ++k)
        q[3 * i + k] = (float)normals[i][k];
    if (!ctx_ || (!normals.empty() && normals.size() != points.size()) ||
        !reported(vr_map_to_points(ctx_, v.data(), (uint32_t)v.size(), p.data(), q.empty() ? nullptr : q.data(),
                                   (uint32_t)points.size(), radius, raw.data())))
      raw.clear();
    return std::vector<NumericType>(raw.begin(), raw.end());
  }

  // ---- closest-hit queries for the caller's rays (not in the reference; vr_cast_rays*, whose header comment has the
  //      definition): each ray traced as apply() traces one — the closest primitive, the side walls followed by their
  //      boundary conditions up to setMaxBoundaryHits — and reported as primitive id, path length, end point and walls
  //      passed.  Directions are used as given, not normalised: distances and tmax are in units of the direction's length.
  //      Needs what apply() leaves behind for the geometry, boundary conditions and source direction in force, and changes
  //      none of it.
  /// the host form: false (with the library's message on std::cerr, `out` emptied) if it was refused
  bool castRays(const std::vector<Vec3D<NumericType>> &origins, const std::vector<Vec3D<NumericType>> &directions,
                CastResult<NumericType> &out, NumericType tmax = std::numeric_limits<NumericType>::infinity(),
                bool followBoundaries = true) {
    const size_t m = origins.size();
    std::vector<float> o(3 * m), d(3 * directions.size()), dist(m), hit(3 * m);
    std::vector<int32_t> prim(m);
    std::vector<uint32_t> bh(m);
    for (size_t i = 0; i < m; ++i)
      for (int k = 0; k < 3; ++k)
        o[3 * i + k] = (float)origins[i][k];
    for (size_t i = 0; i < directions.size(); ++i)
      for (int k = 0; k < 3; ++k)
        d[3 * i + k] = (float)directions[i][k];
    out = CastResult<NumericType>{};
    if (!ctx_ || directions.size() != m ||
        !reported(vr_cast_rays(ctx_, o.data(), d.data(), (uint32_t)m, 1e-4f, (float)tmax,
                               followBoundaries ? VR_CAST_FOLLOW_BOUNDARIES : 0u, prim.data(), dist.data(), hit.data(), bh.data())))
      return false;
    out.primIDs.assign(prim.begin(), prim.end());
    out.distances.assign(dist.begin(), dist.end());
    out.boundaryHits.assign(bh.begin(), bh.end());
    out.hitPoints.resize(m);
    for (size_t i = 0; i < m; ++i)
      for (int k = 0; k < 3; ++k)
        out.hitPoints[i][k] = (NumericType)hit[3 * i + k];
    return true;
  }
  /// dOrg / dDir (m rows of ld = 2 or 3 floats, 2 only with D == 2), dPrim (m int32), dDist (m floats), dHit (nullptr or
  /// m x 3 floats) and dBh (nullptr or m uint32) are DEVICE memory; flags: VR_CAST_FOLLOW_BOUNDARIES or 0; tnear as the
  /// tracer's (1e-4); getFluxDevice's stream rules.  false if it was refused.
  bool castRaysDevice(const float *dOrg, const float *dDir, size_t m, unsigned ld, float tmax, unsigned flags, int32_t *dPrim,
                      float *dDist, float *dHit = nullptr, uint32_t *dBh = nullptr, void *stream = nullptr) {
    return ctx_ && reported(vr_cast_rays_device(ctx_, dOrg, dDir, (uint32_t)m, ld, 1e-4f, tmax, flags, dPrim, dDist, dHit, dBh,
                                                stream));
  }

  // ---- gather flux (not in the reference; vr_gather_flux*, whose header comment has the definition): the flux every
  //      primitive receives straight from the source, estimated by `samples` rays cast FROM the primitive into its own
  //      hemisphere — the same number for every primitive, whatever its depth.  SOURCE-normalised: an unoccluded primitive
  //      facing the source is 1, exactly so for cosinePower 1.  With `emission` (one value per primitive: incoming flux x
  //      reflectivity) a sample that lands on another primitive's front brings that value back: one radiosity iteration.
  //      Needs what apply() leaves behind, like castRays, and changes none of it.
  /// empty, with the library's message on std::cerr, if it was refused
  [[nodiscard]] std::vector<NumericType> gatherFlux(unsigned samples, NumericType cosinePower = 1,
                                                    GatherMode mode = GatherMode::NORMAL,
                                                    const std::vector<NumericType> *emission = nullptr) {
    if (!ctx_)
      return {};
    const uint32_t n = vr_num_primitives(ctx_);
    std::vector<float> e, raw(n);
    if (emission)
      e.assign(emission->begin(), emission->end());
    if (emission && e.size() != n) {
      std::cerr << "viennaray_amd: gatherFlux: emission has " << e.size() << " entries, the scene " << n << " primitives\n";
      return {};
    }
    if (!reported(vr_gather_flux(ctx_, 0u, n, samples, (float)cosinePower, (uint32_t)mode, emission ? e.data() : nullptr, raw.data())))
      return {};
    return std::vector<NumericType>(raw.begin(), raw.end());
  }
  /// dEmission (nullptr or numPrimitives floats) and dOut (primCount floats) are DEVICE memory; getFluxDevice's stream
  /// rules.  false if it was refused.
  bool gatherFluxDevice(unsigned primFirst, unsigned primCount, unsigned samples, float cosinePower, GatherMode mode,
                        const float *dEmission, float *dOut, void *stream = nullptr) {
    return ctx_ && reported(vr_gather_flux_device(ctx_, primFirst, primCount, samples, cosinePower, (uint32_t)mode, dEmission,
                                                  dOut, stream));
  }

  // ---- path gather (not in the reference; vr_gather_paths*, whose header comment has the definition): gatherFlux's
  //      samples followed through their reflections until they reach the source plane — the multi-bounce incoming flux of
  //      a species that reflects specularly (or is re-emitted diffusely) with probability 1 - sticking, with the same
  //      number of samples for every primitive.  SOURCE-normalised like gatherFlux; maxBounces = 0 is gatherFlux(samples).
  /// empty, with the library's message on std::cerr, if it was refused
  [[nodiscard]] std::vector<NumericType> gatherPaths(unsigned samples, NumericType sticking,
                                                     GatherReflection reflection = GatherReflection::SPECULAR,
                                                     unsigned maxBounces = 64, NumericType cosinePower = 1) {
    return gatherPathsImpl(samples, nullptr, 1.f - (float)sticking, reflection, maxBounces, cosinePower);
  }
  /// ... with one sticking value per primitive
  [[nodiscard]] std::vector<NumericType> gatherPaths(unsigned samples, const std::vector<NumericType> &sticking,
                                                     GatherReflection reflection = GatherReflection::SPECULAR,
                                                     unsigned maxBounces = 64, NumericType cosinePower = 1) {
    std::vector<float> rho(sticking.size());
    for (size_t i = 0; i < rho.size(); ++i)
      rho[i] = 1.f - (float)sticking[i];
    if (!ctx_ || rho.size() != vr_num_primitives(ctx_)) {
      std::cerr << "viennaray_amd: gatherPaths: sticking has " << rho.size() << " entries, the scene "
                << (ctx_ ? vr_num_primitives(ctx_) : 0u) << " primitives\n";
      return {};
    }
    return gatherPathsImpl(samples, rho.data(), 0.f, reflection, maxBounces, cosinePower);
  }
  /// dReflectivity (nullptr: reflectivityScalar counts; else numPrimitives floats) and dOut (primCount floats) are DEVICE
  /// memory; getFluxDevice's stream rules.  false if it was refused.
  bool gatherPathsDevice(unsigned primFirst, unsigned primCount, unsigned samples, float cosinePower, GatherReflection reflection,
                         unsigned maxBounces, const float *dReflectivity, float reflectivityScalar, float *dOut,
                         void *stream = nullptr) {
    return ctx_ && reported(vr_gather_paths_device(ctx_, primFirst, primCount, samples, cosinePower, (uint32_t)reflection,
                                                   maxBounces, dReflectivity, reflectivityScalar, dOut, stream));
  }

  // ---- gather to a target error (not in the reference; vr_gather_sums* / vr_gather_adaptive*, whose header comment has
  //      the definition): every primitive starts with minSamples samples and doubles its own count until the standard
  //      error of its mean is at most max(relTarget x mean, absTarget), or maxSamples is reached.  flux[i] has the bits of
  //      the fixed-K call at K = samplesUsed[i].
  /// what an adaptive gather returns: one entry per primitive, and the call's info; empty vectors if it was refused
  struct GatherAdaptiveResult {
    std::vector<NumericType> flux, stdErr;
    std::vector<unsigned> samplesUsed;
    vr_gather_adaptive_info info{};
  };
  [[nodiscard]] GatherAdaptiveResult gatherFluxAdaptive(NumericType relTarget, unsigned minSamples = 64, unsigned maxSamples = 4096,
                                                        NumericType absTarget = 0, NumericType cosinePower = 1,
                                                        GatherMode mode = GatherMode::NORMAL,
                                                        const std::vector<NumericType> *emission = nullptr) {
    std::vector<float> e;
    if (emission)
      e.assign(emission->begin(), emission->end());
    if (ctx_ && emission && e.size() != vr_num_primitives(ctx_)) {
      std::cerr << "viennaray_amd: gatherFluxAdaptive: emission has " << e.size() << " entries, the scene "
                << vr_num_primitives(ctx_) << " primitives\n";
      return {};
    }
    vr_gather_spec spec{};
    spec.cosinePower = (float)cosinePower;
    spec.mode = (uint32_t)mode;
    spec.emission = emission ? e.data() : nullptr;
    return gatherAdaptiveImpl(spec, relTarget, absTarget, minSamples, maxSamples);
  }
  [[nodiscard]] GatherAdaptiveResult gatherPathsAdaptive(NumericType relTarget, NumericType sticking,
                                                         GatherReflection reflection = GatherReflection::SPECULAR,
                                                         unsigned maxBounces = 64, unsigned minSamples = 64,
                                                         unsigned maxSamples = 4096, NumericType absTarget = 0,
                                                         NumericType cosinePower = 1) {
    return gatherAdaptiveImpl(pathsSpec(nullptr, 1.f - (float)sticking, reflection, maxBounces, cosinePower), relTarget, absTarget,
                              minSamples, maxSamples);
  }
  /// the spec's tables and the outputs (dFlux: primCount floats; dStdErr, dSamplesUsed: nullptr or primCount entries) are
  /// DEVICE memory, info is the host's; getFluxDevice's stream rules, the host waits for one word per round.  false if it
  /// was refused.
  bool gatherAdaptiveDevice(const vr_gather_spec &spec, unsigned primFirst, unsigned primCount, unsigned minSamples,
                            unsigned maxSamples, float relTarget, float absTarget, float *dFlux, float *dStdErr,
                            uint32_t *dSamplesUsed, vr_gather_adaptive_info &info, void *stream = nullptr) {
    return ctx_ && reported(vr_gather_adaptive_device(ctx_, &spec, primFirst, primCount, minSamples, maxSamples, relTarget,
                                                      absTarget, dFlux, dStdErr, dSamplesUsed, &info, stream));
  }
  /// the exact int64 sums of the quantised weights (2^-40) and of their squares (2^-28) over chunks [chunkFirst,
  /// chunkFirst + chunks) of a call of `budget` samples, per primitive (host tables in the spec).  false if it was refused.
  bool gatherSums(const vr_gather_spec &spec, unsigned chunkFirst, unsigned chunks, unsigned budget, std::vector<int64_t> &sum,
                  std::vector<int64_t> &sumSq) {
    if (!ctx_)
      return false;
    const uint32_t n = vr_num_primitives(ctx_);
    sum.assign(n, 0);
    sumSq.assign(n, 0);
    return reported(vr_gather_sums(ctx_, &spec, 0u, n, chunkFirst, chunks, budget, sum.data(), sumSq.data()));
  }
  /// the spec of a gatherPaths sample (reflectivity: nullptr or numPrimitives values the caller keeps alive)
  static vr_gather_spec pathsSpec(const float *reflectivity, float reflectivityScalar, GatherReflection reflection,
                                  unsigned maxBounces, NumericType cosinePower = 1) {
    vr_gather_spec spec{};
    spec.cosinePower = (float)cosinePower;
    spec.mode = VR_GATHER_NORMAL;
    spec.paths = 1u;
    spec.reflection = (uint32_t)reflection;
    spec.maxBounces = maxBounces;
    spec.reflectivity = reflectivity;
    spec.reflectivityScalar = reflectivityScalar;
    return spec;
  }

  // ---- angular gather (not in the reference; vr_gather_angular*, whose header comment has the definition): gatherPaths
  //      with up to three tabulated laws of a cosine in [0, 1] — the source's radiance L(c), the reflectivity R(mu) by the
  //      cosine of incidence, the yield Y(mu0) by the sample's own starting angle.  With no law, or all-ones laws, the
  //      results are gatherPaths's word for word.
  /// the laws of an angular gather: each empty (absent) or 2 .. 256 values, nodes at k / (M - 1); the object must outlive
  /// the vr_gather_laws taken from it
  struct GatherLaws {
    std::vector<float> source, reflectivity, yield;
    [[nodiscard]] vr_gather_laws pod() const {
      vr_gather_laws l{};
      l.sourceLaw = source.empty() ? nullptr : source.data();
      l.sourceCount = (uint32_t)source.size();
      l.reflectivityLaw = reflectivity.empty() ? nullptr : reflectivity.data();
      l.reflectivityCount = (uint32_t)reflectivity.size();
      l.yieldLaw = yield.empty() ? nullptr : yield.data();
      l.yieldCount = (uint32_t)yield.size();
      return l;
    }
  };
  /// one value per primitive (empty if it was refused); sticking: the scalar of gatherPaths
  [[nodiscard]] std::vector<NumericType> gatherAngular(unsigned samples, const GatherLaws &laws, NumericType sticking,
                                                       GatherReflection reflection = GatherReflection::SPECULAR,
                                                       unsigned maxBounces = 64, NumericType cosinePower = 1) {
    if (!ctx_)
      return {};
    const vr_gather_spec spec = pathsSpec(nullptr, 1.f - (float)sticking, reflection, maxBounces, cosinePower);
    const vr_gather_laws l = laws.pod();
    std::vector<float> raw(vr_num_primitives(ctx_));
    if (!reported(vr_gather_angular(ctx_, &spec, &l, 0u, (uint32_t)raw.size(), samples, raw.data())))
      return {};
    return std::vector<NumericType>(raw.begin(), raw.end());
  }
  /// spec.reflectivity and dOut (primCount floats) are DEVICE memory, the laws the host's; gatherPathsDevice's stream rules
  bool gatherAngularDevice(const vr_gather_spec &spec, const GatherLaws &laws, unsigned primFirst, unsigned primCount,
                           unsigned samples, float *dOut, void *stream = nullptr) {
    const vr_gather_laws l = laws.pod();
    return ctx_ && reported(vr_gather_angular_device(ctx_, &spec, &l, primFirst, primCount, samples, dOut, stream));
  }
  [[nodiscard]] GatherAdaptiveResult gatherAngularAdaptive(NumericType relTarget, const GatherLaws &laws, NumericType sticking,
                                                           GatherReflection reflection = GatherReflection::SPECULAR,
                                                           unsigned maxBounces = 64, unsigned minSamples = 64,
                                                           unsigned maxSamples = 4096, NumericType absTarget = 0,
                                                           NumericType cosinePower = 1) {
    if (!ctx_)
      return {};
    const vr_gather_spec spec = pathsSpec(nullptr, 1.f - (float)sticking, reflection, maxBounces, cosinePower);
    const vr_gather_laws l = laws.pod();
    const uint32_t n = vr_num_primitives(ctx_);
    std::vector<float> flux(n), err(n);
    GatherAdaptiveResult r;
    r.samplesUsed.resize(n);
    if (!reported(vr_gather_angular_adaptive(ctx_, &spec, &l, 0u, n, minSamples, maxSamples, (float)relTarget, (float)absTarget,
                                             flux.data(), err.data(), reinterpret_cast<uint32_t *>(r.samplesUsed.data()), &r.info)))
      return {};
    r.flux.assign(flux.begin(), flux.end());
    r.stdErr.assign(err.begin(), err.end());
    return r;
  }
  bool gatherAngularAdaptiveDevice(const vr_gather_spec &spec, const GatherLaws &laws, unsigned primFirst, unsigned primCount,
                                   unsigned minSamples, unsigned maxSamples, float relTarget, float absTarget, float *dFlux,
                                   float *dStdErr, uint32_t *dSamplesUsed, vr_gather_adaptive_info &info, void *stream = nullptr) {
    const vr_gather_laws l = laws.pod();
    return ctx_ && reported(vr_gather_angular_adaptive_device(ctx_, &spec, &l, primFirst, primCount, minSamples, maxSamples,
                                                              relTarget, absTarget, dFlux, dStdErr, dSamplesUsed, &info, stream));
  }
  /// gatherSums of an angular gather's samples (host tables in the spec).  false if it was refused.
  bool gatherAngularSums(const vr_gather_spec &spec, const GatherLaws &laws, unsigned chunkFirst, unsigned chunks, unsigned budget,
                         std::vector<int64_t> &sum, std::vector<int64_t> &sumSq) {
    if (!ctx_)
      return false;
    const vr_gather_laws l = laws.pod();
    const uint32_t n = vr_num_primitives(ctx_);
    sum.assign(n, 0);
    sumSq.assign(n, 0);
    return reported(vr_gather_angular_sums(ctx_, &spec, &l, 0u, n, chunkFirst, chunks, budget, sum.data(), sumSq.data()));
  }
  /// ONE path of gatherAngular (vr_debug_gather_angular_path): up to maxVertices vertices in ids / data (12 floats each),
  /// how it ended, its throughput and weight.  false if it was refused.
  struct GatherPathRecord {
    std::vector<uint32_t> ids;
    std::vector<float> data;
    uint32_t numVertices = 0, end = 0;
    float direction[3] = {0.f, 0.f, 0.f}, throughput = 0.f, weight = 0.f;
  };
  bool debugGatherAngularPath(const vr_gather_spec &spec, const GatherLaws &laws, unsigned prim, unsigned sample,
                              unsigned maxVertices, GatherPathRecord &rec) {
    if (!ctx_)
      return false;
    const vr_gather_laws l = laws.pod();
    rec.ids.assign(maxVertices, 0u);
    rec.data.assign((size_t)maxVertices * VR_GATHER_PATH_VERTEX_FLOATS, 0.f);
    return reported(vr_debug_gather_angular_path(ctx_, &spec, &l, prim, sample, maxVertices, rec.ids.data(), rec.data.data(),
                                                 &rec.numVertices, &rec.end, rec.direction, &rec.throughput, &rec.weight));
  }

  // ---- energy gather (not in the reference; vr_gather_energy*, whose header comment has the definition): gatherAngular
  //      with the ion's energy carried along every path — E0 at the source, a share retention(mu) kept at every
  //      reflection, one more multiply by yield(E / energyMax) at the tail.  With an all-ones yield the results are
  //      gatherAngular's word for word.
  /// the energy tables of an energy gather: yield required, quantiles and retention empty (absent) or 2 .. 256 values;
  /// the object must outlive the vr_gather_energy taken from it
  struct GatherEnergy {
    std::vector<float> yield, sourceQuantiles, retention;
    float energyMax = 1.f, sourceEnergy = 0.f; // sourceEnergy counts where sourceQuantiles is empty
    bool energyCut = true;
    [[nodiscard]] struct vr_gather_energy pod() const {
      struct vr_gather_energy e {};
      e.energyYield = yield.empty() ? nullptr : yield.data();
      e.energyYieldCount = (uint32_t)yield.size();
      e.energyMax = energyMax;
      e.sourceQuantiles = sourceQuantiles.empty() ? nullptr : sourceQuantiles.data();
      e.sourceQuantilesCount = (uint32_t)sourceQuantiles.size();
      e.sourceEnergy = sourceEnergy;
      e.retentionLaw = retention.empty() ? nullptr : retention.data();
      e.retentionCount = (uint32_t)retention.size();
      e.energyCut = energyCut ? 1u : 0u;
      return e;
    }
  };
  /// one value per primitive (empty if it was refused); sticking: the scalar of gatherPaths
  [[nodiscard]] std::vector<NumericType> gatherEnergy(unsigned samples, const GatherEnergy &energy, const GatherLaws &laws,
                                                      NumericType sticking, GatherReflection reflection = GatherReflection::SPECULAR,
                                                      unsigned maxBounces = 64, NumericType cosinePower = 1) {
    if (!ctx_)
      return {};
    const vr_gather_spec spec = pathsSpec(nullptr, 1.f - (float)sticking, reflection, maxBounces, cosinePower);
    const vr_gather_laws l = laws.pod();
    const struct vr_gather_energy e = energy.pod();
    std::vector<float> raw(vr_num_primitives(ctx_));
    if (!reported(::vr_gather_energy(ctx_, &spec, &l, &e, 0u, (uint32_t)raw.size(), samples, raw.data())))
      return {};
    return std::vector<NumericType>(raw.begin(), raw.end());
  }
  /// spec.reflectivity and dOut (primCount floats) are DEVICE memory, the tables the host's; gatherPathsDevice's stream rules
  bool gatherEnergyDevice(const vr_gather_spec &spec, const GatherLaws &laws, const GatherEnergy &energy, unsigned primFirst,
                          unsigned primCount, unsigned samples, float *dOut, void *stream = nullptr) {
    const vr_gather_laws l = laws.pod();
    const struct vr_gather_energy e = energy.pod();
    return ctx_ && reported(vr_gather_energy_device(ctx_, &spec, &l, &e, primFirst, primCount, samples, dOut, stream));
  }
  /// gatherSums of an energy gather's samples (host tables in the spec).  false if it was refused.
  bool gatherEnergySums(const vr_gather_spec &spec, const GatherLaws &laws, const GatherEnergy &energy, unsigned chunkFirst,
                        unsigned chunks, unsigned budget, std::vector<int64_t> &sum, std::vector<int64_t> &sumSq) {
    if (!ctx_)
      return false;
    const vr_gather_laws l = laws.pod();
    const struct vr_gather_energy e = energy.pod();
    const uint32_t n = vr_num_primitives(ctx_);
    sum.assign(n, 0);
    sumSq.assign(n, 0);
    return reported(vr_gather_energy_sums(ctx_, &spec, &l, &e, 0u, n, chunkFirst, chunks, budget, sum.data(), sumSq.data()));
  }
  [[nodiscard]] GatherAdaptiveResult gatherEnergyAdaptive(NumericType relTarget, const GatherEnergy &energy, const GatherLaws &laws,
                                                          NumericType sticking,
                                                          GatherReflection reflection = GatherReflection::SPECULAR,
                                                          unsigned maxBounces = 64, unsigned minSamples = 64,
                                                          unsigned maxSamples = 4096, NumericType absTarget = 0,
                                                          NumericType cosinePower = 1) {
    if (!ctx_)
      return {};
    const vr_gather_spec spec = pathsSpec(nullptr, 1.f - (float)sticking, reflection, maxBounces, cosinePower);
    const vr_gather_laws l = laws.pod();
    const struct vr_gather_energy e = energy.pod();
    const uint32_t n = vr_num_primitives(ctx_);
    std::vector<float> flux(n), err(n);
    GatherAdaptiveResult r;
    r.samplesUsed.resize(n);
    if (!reported(vr_gather_energy_adaptive(ctx_, &spec, &l, &e, 0u, n, minSamples, maxSamples, (float)relTarget, (float)absTarget,
                                            flux.data(), err.data(), reinterpret_cast<uint32_t *>(r.samplesUsed.data()), &r.info)))
      return {};
    r.flux.assign(flux.begin(), flux.end());
    r.stdErr.assign(err.begin(), err.end());
    return r;
  }

  // ---- species gather (not in the reference; vr_gather_species*, whose header comment has the definition): up to
  //      VR_GATHER_MAX_SPECIES species weighed along ONE set of traced paths.  Row s of the result is gatherAngular of
  //      species s word for word; reflection and maxBounces make the path and are shared.
  /// one species: gatherAngular's per-species arguments.  reflectivity: empty (the scalar 1 - sticking counts) or one value
  /// per primitive; the object must outlive the call
  struct GatherSpecies {
    NumericType sticking = 1;
    std::vector<float> reflectivity;
    NumericType cosinePower = 1;
    GatherLaws laws;
  };
  /// row-major [species][primitive] (empty if it was refused)
  [[nodiscard]] std::vector<NumericType> gatherSpecies(unsigned samples, const std::vector<GatherSpecies> &species,
                                                       GatherReflection reflection = GatherReflection::SPECULAR,
                                                       unsigned maxBounces = 64) {
    if (!ctx_)
      return {};
    std::vector<vr_gather_spec> specs;
    std::vector<vr_gather_laws> laws;
    speciesPods(species, reflection, maxBounces, specs, laws);
    std::vector<float> raw(species.size() * (size_t)vr_num_primitives(ctx_));
    if (!reported(vr_gather_species(ctx_, specs.data(), laws.data(), (uint32_t)species.size(), 0u, vr_num_primitives(ctx_), samples,
                                    raw.data())))
      return {};
    return std::vector<NumericType>(raw.begin(), raw.end());
  }
  /// specs[s].reflectivity and dOut (numSpecies x primCount floats) are DEVICE memory, the laws the host's (nullptr: none);
  /// gatherPathsDevice's stream rules
  bool gatherSpeciesDevice(const std::vector<vr_gather_spec> &specs, const vr_gather_laws *laws, unsigned primFirst,
                           unsigned primCount, unsigned samples, float *dOut, void *stream = nullptr) {
    return ctx_ && reported(vr_gather_species_device(ctx_, specs.data(), laws, (uint32_t)specs.size(), primFirst, primCount, samples,
                                                     dOut, stream));
  }
  /// gatherAngularSums for every species along one set of paths: sum, sumSq row-major [species][primitive].  false if it
  /// was refused.
  bool gatherSpeciesSums(const std::vector<GatherSpecies> &species, GatherReflection reflection, unsigned maxBounces,
                         unsigned chunkFirst, unsigned chunks, unsigned budget, std::vector<int64_t> &sum,
                         std::vector<int64_t> &sumSq) {
    if (!ctx_)
      return false;
    std::vector<vr_gather_spec> specs;
    std::vector<vr_gather_laws> laws;
    speciesPods(species, reflection, maxBounces, specs, laws);
    const uint32_t n = vr_num_primitives(ctx_);
    sum.assign(species.size() * (size_t)n, 0);
    sumSq.assign(species.size() * (size_t)n, 0);
    return reported(vr_gather_species_sums(ctx_, specs.data(), laws.data(), (uint32_t)species.size(), 0u, n, chunkFirst, chunks, budget,
                                           sum.data(), sumSq.data()));
  }
  /// what an adaptive species gather returns: flux, stdErr and samplesUsed row-major [species][primitive], and the call's
  /// info; empty vectors if it was refused
  struct GatherSpeciesAdaptiveResult {
    std::vector<NumericType> flux, stdErr;
    std::vector<unsigned> samplesUsed;
    vr_gather_species_adaptive_info info{};
  };
  /// gatherSpecies to a target error per species (vr_gather_species_adaptive, whose header comment has the definition):
  /// row s is gatherAngularAdaptive of species s under relTargets[s] / absTargets[s] word for word, along one set of
  /// traced paths.  relTargets: one value per species; absTargets: one per species, or empty (all 0)
  [[nodiscard]] GatherSpeciesAdaptiveResult gatherSpeciesAdaptive(const std::vector<float> &relTargets,
                                                                  const std::vector<GatherSpecies> &species,
                                                                  GatherReflection reflection = GatherReflection::SPECULAR,
                                                                  unsigned maxBounces = 64, unsigned minSamples = 64,
                                                                  unsigned maxSamples = 4096, std::vector<float> absTargets = {}) {
    if (!ctx_)
      return {};
    if (absTargets.empty())
      absTargets.assign(species.size(), 0.f);
    if (relTargets.size() != species.size() || absTargets.size() != species.size()) {
      std::cerr << "viennaray_amd: gatherSpeciesAdaptive: " << species.size() << " species, " << relTargets.size()
                << " relative and " << absTargets.size() << " absolute targets\n";
      return {};
    }
    std::vector<vr_gather_spec> specs;
    std::vector<vr_gather_laws> laws;
    speciesPods(species, reflection, maxBounces, specs, laws);
    const size_t n = species.size() * (size_t)vr_num_primitives(ctx_);
    std::vector<float> flux(n), err(n);
    GatherSpeciesAdaptiveResult r;
    r.samplesUsed.resize(n);
    if (!reported(vr_gather_species_adaptive(ctx_, specs.data(), laws.data(), (uint32_t)species.size(), 0u, vr_num_primitives(ctx_),
                                             minSamples, maxSamples, relTargets.data(), absTargets.data(), flux.data(), err.data(),
                                             reinterpret_cast<uint32_t *>(r.samplesUsed.data()), &r.info)))
      return {};
    r.flux.assign(flux.begin(), flux.end());
    r.stdErr.assign(err.begin(), err.end());
    return r;
  }
  /// specs[s].reflectivity and the outputs (dFlux: numSpecies x primCount floats; dStdErr, dSamplesUsed: nullptr or as many
  /// entries) are DEVICE memory; the laws (nullptr: none), the targets (numSpecies floats each) and info are the host's;
  /// gatherAdaptiveDevice's stream rules.  false if it was refused.
  bool gatherSpeciesAdaptiveDevice(const std::vector<vr_gather_spec> &specs, const vr_gather_laws *laws, unsigned primFirst,
                                   unsigned primCount, unsigned minSamples, unsigned maxSamples, const float *relTargets,
                                   const float *absTargets, float *dFlux, float *dStdErr, uint32_t *dSamplesUsed,
                                   vr_gather_species_adaptive_info &info, void *stream = nullptr) {
    return ctx_ && reported(vr_gather_species_adaptive_device(ctx_, specs.data(), laws, (uint32_t)specs.size(), primFirst, primCount,
                                                              minSamples, maxSamples, relTargets, absTargets, dFlux, dStdErr,
                                                              dSamplesUsed, &info, stream));
  }
  /// the specs and laws of a list of species (host tables; the species must outlive them)
  static void speciesPods(const std::vector<GatherSpecies> &species, GatherReflection reflection, unsigned maxBounces,
                          std::vector<vr_gather_spec> &specs, std::vector<vr_gather_laws> &laws) {
    specs.clear();
    laws.clear();
    for (const GatherSpecies &s : species) {
      specs.push_back(pathsSpec(s.reflectivity.empty() ? nullptr : s.reflectivity.data(), 1.f - (float)s.sticking, reflection,
                                maxBounces, s.cosinePower));
      laws.push_back(s.laws.pod());
    }
  }

  // ---- radiosity solve (not in the reference; vr_radiosity_*, whose header comment has the definition): the
  //      steady-state incoming flux of a species re-emitted diffusely with probability 1 - sticking — the fixed point of
  //      gatherFlux(samples, emission = (1 - sticking) x flux).  The samples are walked once into a link table that stays
  //      resident and is reused while samples, cosinePower and the scene's settings stay as they are; every iteration is
  //      a pass over that table.  SOURCE-normalised like gatherFlux.
  /// what the solve did beyond the flux
  struct RadiosityInfo {
    unsigned iterations = 0;
    float residual = 0.f;
  };
  /// empty, with the library's message on std::cerr, if it was refused; the table is built when none matches
  [[nodiscard]] std::vector<NumericType> solveRadiosity(unsigned samples, NumericType sticking, NumericType cosinePower = 1,
                                                        NumericType tolerance = NumericType(1e-4), unsigned maxIterations = 1000,
                                                        RadiosityInfo *info = nullptr) {
    return solveRadiosityImpl(samples, nullptr, 1.f - (float)sticking, cosinePower, tolerance, maxIterations, info);
  }
  /// ... with one sticking value per primitive
  [[nodiscard]] std::vector<NumericType> solveRadiosity(unsigned samples, const std::vector<NumericType> &sticking,
                                                        NumericType cosinePower = 1, NumericType tolerance = NumericType(1e-4),
                                                        unsigned maxIterations = 1000, RadiosityInfo *info = nullptr) {
    std::vector<float> rho(sticking.size());
    for (size_t i = 0; i < rho.size(); ++i)
      rho[i] = 1.f - (float)sticking[i];
    if (!ctx_ || rho.size() != vr_num_primitives(ctx_)) {
      std::cerr << "viennaray_amd: solveRadiosity: sticking has " << rho.size() << " entries, the scene "
                << (ctx_ ? vr_num_primitives(ctx_) : 0u) << " primitives\n";
      return {};
    }
    return solveRadiosityImpl(samples, rho.data(), 0.f, cosinePower, tolerance, maxIterations, info);
  }
  /// build or replace the link table (solveRadiosity does it when none matches); false if it was refused
  bool radiosityLinks(unsigned samples, float cosinePower = 1.f, void *stream = nullptr) {
    return ctx_ && reported(vr_radiosity_links_device(ctx_, samples, cosinePower, stream));
  }
  [[nodiscard]] uint64_t radiosityLinkBytes(unsigned samples) const { return ctx_ ? vr_radiosity_link_bytes(ctx_, samples) : 0; }
  void freeRadiosityLinks() {
    if (ctx_)
      check(vr_radiosity_free_links(ctx_));
  }
  /// dReflectivity (nullptr: reflectivityScalar counts; else numPrimitives floats) and dOut (numPrimitives floats) are
  /// DEVICE memory; needs a table (radiosityLinks); getFluxDevice's stream rules.  false if it was refused.
  bool solveRadiosityDevice(const float *dReflectivity, float reflectivityScalar, float tolerance, unsigned maxIterations,
                            float *dOut, RadiosityInfo *info = nullptr, void *stream = nullptr) {
    uint32_t its = 0;
    float res = 0.f;
    if (!ctx_ || !reported(vr_radiosity_solve_device(ctx_, dReflectivity, reflectivityScalar, tolerance, maxIterations, dOut, &its,
                                                     &res, stream)))
      return false;
    if (info)
      *info = RadiosityInfo{its, res};
    return true;
  }

  // ---- flux statistics (not in the reference; vr_set_flux_statistics): per-primitive hit counts and the Monte-Carlo
  //      error of the flux label.  A per-credit estimator: it ignores the correlation between several credits of one ray
  //      to the same primitive.  Off by default; an absorbing particle keeps its kernels, every other launch runs the
  //      extended kernels with the statistics compiled in.  With statistics on a particle has at most two data labels.
  void setCalculateFluxError(const bool on) {
    if (ctx_)
      check(vr_set_flux_statistics(ctx_, on ? 1 : 0));
  }
  /// credits to the flux label of every primitive in the last apply (particle `particleIdx` of a particle list);
  /// empty, with the library's message on std::cerr, if the getter was refused (statistics off, no apply yet)
  [[nodiscard]] std::vector<uint64_t> getHitCounts(unsigned particleIdx = 0) {
    std::vector<uint64_t> out(ctx_ ? vr_num_primitives(ctx_) : 0);
    if (!ctx_ || !reported(vr_get_hit_counts(ctx_, particleIdx, out.data(), (uint32_t)out.size())))
      out.clear();
    return out;
  }
  /// sigma / S1 per primitive, +inf where nothing was credited; the same for every NormalizationType
  [[nodiscard]] std::vector<NumericType> getFluxRelativeError(unsigned particleIdx = 0) { return fluxError(particleIdx, 0); }
  /// sigma = sqrt(max(sumsq - S1^2 / N, 0)) per primitive, in raw flux units; N: the rays of the whole apply
  [[nodiscard]] std::vector<NumericType> getFluxAbsoluteError(unsigned particleIdx = 0) { return fluxError(particleIdx, 1); }
  /// ... written to DEVICE memory `dOut` (float32, one per primitive) under getFluxDevice's stream rules; false if refused
  bool getFluxErrorDevice(float *dOut, unsigned particleIdx = 0, bool relative = true, void *stream = nullptr) {
    return ctx_ && reported(vr_get_flux_error_device(ctx_, particleIdx, relative ? 0 : 1, dOut, vr_num_primitives(ctx_), stream));
  }

  [[nodiscard]] TracingData<NumericType> &getLocalData() { return localData_; }
  // rayTrace.hpp:137-145: global data is a borrowed pointer handed to user particles; apply() copies its vectors and
  // scalars to the device, where the registry's particle models read them (ModelCtx::global)
  [[nodiscard]] TracingData<NumericType> *getGlobalData() { return pGlobalData_; }
  void setGlobalData(TracingData<NumericType> &data) {
    pGlobalData_ = &data;
    deviceGlobal_ = 0; // (the borrowed data is the global data again, all of it)
  }
  /// Vector `vecIdx` of the global data from DEVICE memory (vr_set_global_data_device): n floats produced on `stream`
  /// (the caller's hipStream_t, nullptr = the null stream), copied into place on the device; the buffer is free for work
  /// queued on `stream` afterwards.  The index then belongs to the device: apply() leaves it alone, whatever the
  /// borrowed TracingData holds at that index, until setGlobalData(TracingData &) is called again.  dData == nullptr or
  /// n == 0 drops the vector and those behind it.
  void setGlobalDataDevice(unsigned vecIdx, const float *dData, size_t n, void *stream = nullptr) {
    if (!deviceCall(false, vr_set_global_data_device, vecIdx, dData, n, stream))
      return;
    if (dData && n)
      deviceGlobal_ |= 1u << vecIdx;
    else
      deviceGlobal_ &= (1u << vecIdx) - 1u;
  }
  [[nodiscard]] TraceInfo getRayTraceInfo() const { return RTInfo_; }
  [[nodiscard]] DataLog<NumericType> &getDataLog() { return dataLog_; }
  /// the underlying C-ABI context (multi-GPU drivers use vr_set_ray_range etc.)
  [[nodiscard]] vr_context *getContext() { return ctx_; }

protected:
  // The data log of this apply: the shape of dataLog_.data as the caller sized it, if a particle's device model has a
  // log_data hook; otherwise (an empty log, or particles that log nothing, like the reference's built-in ones) no shape:
  // nothing is logged and nothing is paid.
  bool setDataLogShape() {
    bool hook = false;
    for (int32_t kind : particleKinds_) {
      int32_t rows = 0;
      hook = hook || (vr_get_model_log_rows(ctx_, kind, &rows) == VR_OK && rows > 0);
    }
    std::vector<uint32_t> sizes;
    if (hook)
      for (const auto &row : dataLog_.data)
        sizes.push_back((uint32_t)row.size());
    check(vr_set_data_log_shape(ctx_, sizes.data(), (uint32_t)sizes.size()));
    return !sizes.empty();
  }
  void mergeDataLog() {
    std::size_t n = 0;
    for (const auto &row : dataLog_.data)
      n += row.size();
    std::vector<float> flat(n);
    if (vr_get_data_log(ctx_, flat.data(), (uint32_t)n) != VR_OK)
      return;
    std::size_t o = 0;
    for (auto &row : dataLog_.data)
      for (auto &v : row)
        v += (NumericType)flat[o++];
  }
  void check(int rc) {
    if (rc != VR_OK) {
      setterError_ = true;
      RTInfo_.error = true;
      std::cerr << "viennaray_amd: " << vr_last_error(ctx_) << "\n";
    }
  }
  // a getter's result: refused -> the library's message on std::cerr (the trace's error flag is a setter's business)
  bool reported(int rc) {
    if (rc != VR_OK)
      std::cerr << "viennaray_amd: " << vr_last_error(ctx_) << "\n";
    return rc == VR_OK;
  }
  // rho: nullptr (the scalar counts) or numPrimitives reflectivities
  std::vector<NumericType> solveRadiosityImpl(unsigned samples, const float *rho, float rhoScalar, NumericType cosinePower,
                                              NumericType tolerance, unsigned maxIterations, RadiosityInfo *info) {
    if (!ctx_)
      return {};
    if (!vr_radiosity_resident(ctx_, samples, (float)cosinePower) &&
        !reported(vr_radiosity_links_device(ctx_, samples, (float)cosinePower, nullptr)))
      return {};
    std::vector<float> raw(vr_num_primitives(ctx_));
    uint32_t its = 0;
    float res = 0.f;
    if (!reported(vr_radiosity_solve(ctx_, rho, rhoScalar, (float)tolerance, maxIterations, raw.data(), &its, &res)))
      return {};
    if (info)
      *info = RadiosityInfo{its, res};
    return std::vector<NumericType>(raw.begin(), raw.end());
  }
  // rho: nullptr (the scalar counts) or numPrimitives reflectivities
  std::vector<NumericType> gatherPathsImpl(unsigned samples, const float *rho, float rhoScalar, GatherReflection reflection,
                                           unsigned maxBounces, NumericType cosinePower) {
    if (!ctx_)
      return {};
    std::vector<float> raw(vr_num_primitives(ctx_));
    if (!reported(vr_gather_paths(ctx_, 0u, (uint32_t)raw.size(), samples, (float)cosinePower, (uint32_t)reflection, maxBounces, rho,
                                  rhoScalar, raw.data())))
      return {};
    return std::vector<NumericType>(raw.begin(), raw.end());
  }
  GatherAdaptiveResult gatherAdaptiveImpl(const vr_gather_spec &spec, NumericType relTarget, NumericType absTarget,
                                          unsigned minSamples, unsigned maxSamples) {
    if (!ctx_)
      return {};
    const uint32_t n = vr_num_primitives(ctx_);
    std::vector<float> flux(n), err(n);
    GatherAdaptiveResult r;
    r.samplesUsed.resize(n);
    static_assert(sizeof(unsigned) == sizeof(uint32_t), "samplesUsed is filled as uint32_t");
    if (!reported(vr_gather_adaptive(ctx_, &spec, 0u, n, minSamples, maxSamples, (float)relTarget, (float)absTarget, flux.data(),
                                     err.data(), reinterpret_cast<uint32_t *>(r.samplesUsed.data()), &r.info)))
      return {};
    r.flux.assign(flux.begin(), flux.end());
    r.stdErr.assign(err.begin(), err.end());
    return r;
  }
  std::vector<NumericType> fluxError(unsigned particleIdx, int kind) {
    std::vector<float> raw(ctx_ ? vr_num_primitives(ctx_) : 0);
    if (!ctx_ || !reported(vr_get_flux_error(ctx_, particleIdx, kind, raw.data(), (uint32_t)raw.size())))
      raw.clear();
    return std::vector<NumericType>(raw.begin(), raw.end());
  }
  bool fluxDevice(float *dOut, int dataIdx, int norm, int numNeighbors, void *stream) {
    if (!ctx_)
      return false;
    const int rc = vr_get_flux_device(ctx_, (uint32_t)dataIdx, dOut, vr_num_primitives(ctx_), norm, numNeighbors, stream);
    if (rc != VR_OK)
      std::cerr << "viennaray_amd: " << vr_last_error(ctx_) << "\n";
    return rc == VR_OK;
  }
  void geometryAccepted(int rc) { // a new geometry clears an earlier refusal
    setterError_ = false;
    check(rc);
  }
  // One of the C ABI's device entry points (vr_*_device), whose last parameter is the caller's stream: the arguments
  // converted to its parameter types, the result checked as a setter's (a geometry's: geometryAccepted).  true if it
  // was accepted; without a context nothing is called.
  template <class... P, class... A> bool deviceCall(bool geometry, int (*entry)(vr_context *, P...), A... args) {
    if (!ctx_)
      return false;
    const int rc = entry(ctx_, static_cast<P>(args)...);
    geometry ? geometryAccepted(rc) : check(rc);
    return rc == VR_OK;
  }
  // rayTrace.hpp:137-145: the borrowed global data may have changed since the last apply — its vectors and scalars
  // go to HBM again (they are what the device particle models read; a few MB at most)
  void uploadGlobalData() {
    if (!ctx_)
      return;
    if (deviceGlobal_) {
      uploadGlobalDataAround();
    } else {
      check(vr_set_global_data(ctx_, 0, nullptr, 0));
      if (pGlobalData_) {
        const auto &vecs = pGlobalData_->getVectorData();
        for (size_t v = 0; v < vecs.size() && v < 16; ++v) {
          std::vector<float> tmp(vecs[v].begin(), vecs[v].end());
          if (!tmp.empty())
            check(vr_set_global_data(ctx_, (uint32_t)v, tmp.data(), (uint32_t)tmp.size()));
        }
      }
    }
    check(vr_set_global_scalars(ctx_, nullptr, 0));
    if (!pGlobalData_)
      return;
    const auto &sc = pGlobalData_->getScalarData();
    std::vector<float> st(sc.begin(), sc.end());
    if (!st.empty())
      check(vr_set_global_scalars(ctx_, st.data(), (uint32_t)st.size()));
  }
  // ... with indices that were set from the device (setGlobalDataDevice): those stay as they are; every other index up
  // to the last one in use gets the borrowed vector, or one zero (which reads as the missing vector does: 0 everywhere)
  // where the borrowed data has none — dropping a vector would take the device-set ones behind it along
  void uploadGlobalDataAround() {
    static const std::vector<std::vector<NumericType>> none;
    const auto &vecs = pGlobalData_ ? pGlobalData_->getVectorData() : none;
    unsigned last = 0;
    for (unsigned v = 0; v < 16; ++v)
      if (((deviceGlobal_ >> v) & 1u) || (v < vecs.size() && !vecs[v].empty()))
        last = v;
    for (unsigned v = 0; v <= last; ++v) {
      if ((deviceGlobal_ >> v) & 1u)
        continue;
      std::vector<float> tmp;
      if (v < vecs.size())
        tmp.assign(vecs[v].begin(), vecs[v].end());
      if (tmp.empty())
        tmp.assign(1, 0.f);
      check(vr_set_global_data(ctx_, v, tmp.data(), (uint32_t)tmp.size()));
    }
    if (last + 1 < 16)
      check(vr_set_global_data(ctx_, last + 1, nullptr, 0));
  }
  // A user Source is a host callback (raySource.hpp:10-19): evaluate it for every ray of the coming
  // apply() exactly as the reference's loop would (rayTraceKernel.hpp:118-140: engine seeded with
  // tea<3>(idx, seed), particle.initNew, source.getOriginAndDirection) and hand the rays over together
  // with the number of engine outputs each consumed.  Needs a fixed seed (setRngSeed).
  bool uploadHostSource() {
    if (useRandomSeeds_) {
      RTInfo_.error = true;
      std::cerr << "viennaray_amd: a host-callback Source needs a fixed seed (setRngSeed): the rays are "
                   "generated on the host before the launch.\n";
      return false;
    }
    uint32_t runNumber = 1;
    vr_get_run_number(ctx_, &runNumber);
    const unsigned seed = runNumber + rngSeed_; // rayTraceKernel.hpp:100
    const size_t perPoint = numRaysPerPoint_, fixed = numRaysFixed_;
    const size_t numRays = fixed ? fixed : pSource_->getNumPoints() * perPoint;
    if (numRays == 0 || numRays > 0xFFFFFFFFull) {
      RTInfo_.error = true;
      std::cerr << "viennaray_amd: host-callback Source: number of rays must be in [1, 2^32).\n";
      return false;
    }
    std::vector<float> org(numRays * 3), dir(numRays * 3), weights(numRays);
    std::vector<uint32_t> draws(numRays);
    bool unitWeights = true;
    auto particle = pParticle_->clone();
    for (size_t idx = 0; idx < numRays; ++idx) {
      weights[idx] = (float)pSource_->getInitialRayWeight(idx); // rayTraceKernel.hpp:124
      unitWeights = unitWeights && weights[idx] == 1.f;
      RNG rng(tea<3>((unsigned)idx, seed));
      particle->initNew(rng);
      auto pd = particle->initNewWithDirection(rng);
      auto od = pSource_->getOriginAndDirection(idx, rng);
      if (pd[0] != NumericType(0) || pd[1] != NumericType(0) || pd[2] != NumericType(0))
        od[1] = pd; // rayTraceKernel.hpp:138-140
      for (int k = 0; k < 3; ++k) {
        org[3 * idx + k] = (float)od[0][k];
        dir[3 * idx + k] = (float)od[1][k];
      }
      draws[idx] = (uint32_t)rng.draws;
    }
    int rc = vr_set_host_rays(ctx_, org.data(), dir.data(), draws.data(), numRays);
    if (rc == VR_OK && !unitWeights)
      rc = vr_set_host_ray_weights(ctx_, weights.data(), numRays);
    if (rc == VR_OK)
      rc = vr_set_source_area(ctx_, (float)pSource_->getSourceArea()); // rayTraceDisk.hpp:127: the source's own area
    if (rc != VR_OK) {
      RTInfo_.error = true;
      std::cerr << vr_last_error(ctx_) << "\n";
      return false;
    }
    return true;
  }
  template <class F> void inPlace(std::vector<NumericType> &flux, F f) {
    if (!ctx_)
      return;
    if constexpr (std::is_same_v<NumericType, float>) {
      if (f(flux.data(), (uint32_t)flux.size()) != VR_OK)
        std::cerr << vr_last_error(ctx_) << "\n";
    } else {
      std::vector<float> tmp(flux.begin(), flux.end());
      if (f(tmp.data(), (uint32_t)tmp.size()) != VR_OK)
        std::cerr << vr_last_error(ctx_) << "\n";
      std::copy(tmp.begin(), tmp.end(), flux.begin());
    }
  }
  template <class Vec> static std::vector<float> flatten3(const std::vector<Vec> &v) {
    std::vector<float> out(v.size() * 3, 0.f);
    for (size_t i = 0; i < v.size(); ++i)
      for (size_t k = 0; k < v[i].size() && k < 3; ++k)
        out[3 * i + k] = (float)v[i][k];
    return out;
  }

  vr_context *ctx_ = nullptr;
  std::unique_ptr<AbstractParticle<NumericType>> pParticle_ = nullptr;
  std::vector<std::unique_ptr<AbstractParticle<NumericType>>> moreParticles_; // setParticleTypes: particles 1 ..
  TracingData<NumericType> localData_;
  TracingData<NumericType> *pGlobalData_ = nullptr;
  unsigned deviceGlobal_ = 0; // bit v: vector v of the global data was set from the device (setGlobalDataDevice)
  DataLog<NumericType> dataLog_;
  std::vector<int32_t> particleKinds_; // the device kinds of pParticle_ and moreParticles_
  std::shared_ptr<Source<NumericType>> pSource_;
  TraceInfo RTInfo_;
  bool particleOnDevice_ = false, sourceOnDevice_ = false, setterError_ = false;
  bool useRandomSeeds_ = true;
  unsigned rngSeed_ = 0;
  size_t numRaysPerPoint_ = 1000, numRaysFixed_ = 0;
  int rank_ = 0, world_ = 1;
  vr_allreduce_fn reduce_ = nullptr;
  void *reduceUser_ = nullptr;
};

template <class NumericType, int D> class TraceDisk final : public Trace<NumericType, D> {
public:
  template <size_t Dim>
  void setGeometry(std::vector<VectorType<NumericType, Dim>> const &points,
                   std::vector<VectorType<NumericType, Dim>> const &normals, const NumericType gridDelta) {
    setGeometry(points, normals, gridDelta, NumericType(0));
  }
  template <size_t Dim>
  void setGeometry(std::vector<VectorType<NumericType, Dim>> const &points,
                   std::vector<VectorType<NumericType, Dim>> const &normals, const NumericType gridDelta,
                   const NumericType diskRadii) {
    static_assert(!(D == 3 && Dim == 2), "Setting 2D geometry in 3D trace object");
    auto p = this->flatten3(points), n = this->flatten3(normals);
    if (this->ctx_)
      this->geometryAccepted(vr_set_disks(this->ctx_, p.data(), n.data(), (uint32_t)points.size(), (float)gridDelta,
                                          (float)diskRadii, D));
  }
  void setGeometry(const DiskMesh &mesh) {
    auto p = this->flatten3(mesh.nodes), n = this->flatten3(mesh.normals);
    if (this->ctx_)
      this->geometryAccepted(vr_set_disks(this->ctx_, p.data(), n.data(), (uint32_t)mesh.nodes.size(), mesh.gridDelta, 0.f, D));
  }
  /// setGeometry for a surface that already lives on the device (vr_set_disks_device): dPoints / dNormals are DEVICE
  /// pointers to n rows of `ld` floats (2 or 3; 2 only for D == 2), produced on `stream` (the caller's hipStream_t,
  /// nullptr = the null stream).  The library takes its own copy on the device: the buffers are free again on return.
  void setGeometryDevice(const float *dPoints, const float *dNormals, size_t n, unsigned ld, NumericType gridDelta,
                         void *stream = nullptr) {
    setGeometryDevice(dPoints, dNormals, n, ld, gridDelta, NumericType(0), stream);
  }
  void setGeometryDevice(const float *dPoints, const float *dNormals, size_t n, unsigned ld, NumericType gridDelta,
                         NumericType diskRadii, void *stream) {
    this->deviceCall(true, vr_set_disks_device, dPoints, dNormals, n, ld, gridDelta, diskRadii, D, stream);
  }
  template <typename T> void setMaterialIds(std::vector<T> const &materialIds) {
    std::vector<int32_t> ids(materialIds.begin(), materialIds.end());
    if (this->ctx_)
      this->check(vr_set_material_ids(this->ctx_, ids.data(), (uint32_t)ids.size()));
  }
};

template <class NumericType, int D> class TraceTriangle final : public Trace<NumericType, D> {
public:
  void setGeometry(std::vector<VectorType<NumericType, 3>> const &points,
                   std::vector<VectorType<unsigned, 3>> const &triangles, const NumericType gridDelta) {
    auto p = this->flatten3(points);
    std::vector<uint32_t> t(triangles.size() * 3);
    for (size_t i = 0; i < triangles.size(); ++i)
      for (int k = 0; k < 3; ++k)
        t[3 * i + k] = triangles[i][k];
    if (this->ctx_)
      this->geometryAccepted(vr_set_triangles(this->ctx_, p.data(), (uint32_t)points.size(), t.data(),
                                              (uint32_t)triangles.size(), (float)gridDelta, D));
  }
  /// setGeometry for a mesh that already lives on the device (vr_set_triangles_device): dVerts is a DEVICE pointer to
  /// nverts rows of 3 floats, dTris one to ntris rows of 3 unsigned, both produced on `stream` (the caller's hipStream_t,
  /// nullptr = the null stream).  The library checks the indices and takes its own copy on the device: the buffers are
  /// free for work queued on `stream` afterwards.
  void setGeometryDevice(const float *dVerts, size_t nverts, const unsigned *dTris, size_t ntris, NumericType gridDelta,
                         void *stream = nullptr) {
    this->deviceCall(true, vr_set_triangles_device, dVerts, nverts, dTris, ntris, gridDelta, D, stream);
  }
  void setGeometry(const TriangleMesh &mesh) {
    std::vector<VectorType<NumericType, 3>> pts(mesh.nodes.size());
    for (size_t i = 0; i < pts.size(); ++i)
      pts[i] = {(NumericType)mesh.nodes[i][0], (NumericType)mesh.nodes[i][1], (NumericType)mesh.nodes[i][2]};
    setGeometry(pts, mesh.triangles, (NumericType)mesh.gridDelta);
  }
  // rayTraceTriangle.hpp:76-81 (2-D only)
  void setGeometry(const LineMesh &mesh) {
    static_assert(D == 2 || D == 3, "dimension");
    setGeometry(convertLinesToTriangles(mesh));
  }
  template <typename T> void setMaterialIds(std::vector<T> const &materialIds) {
    std::vector<int32_t> ids(materialIds.begin(), materialIds.end());
    if (this->ctx_)
      this->check(vr_set_material_ids(this->ctx_, ids.data(), (uint32_t)ids.size()));
  }
};

} // namespace viennaray

namespace rayInternal {
using namespace viennaray;

// file formats: rayUtil.hpp:353-411
template <typename NumericType>
void readGridFromFile(const std::string &fileName, NumericType &gridDelta, std::vector<Vec3D<NumericType>> &points,
                      std::vector<Vec3D<NumericType>> &normals) {
  std::ifstream f(fileName);
  if (!f.is_open()) {
    std::cout << "Cannot read file " << fileName << std::endl;
    return;
  }
  size_t n;
  f >> n >> gridDelta;
  points.resize(n);
  normals.resize(n);
  for (auto &p : points)
    f >> p[0] >> p[1] >> p[2];
  for (auto &p : normals)
    f >> p[0] >> p[1] >> p[2];
}

template <typename NumericType, int D>
void readMeshFromFile(const std::string &fileName, NumericType &gridDelta, std::vector<Vec3D<NumericType>> &nodes,
                      std::vector<VectorType<unsigned, D>> &elements) {
  std::ifstream f(fileName);
  if (!f.is_open()) {
    std::cerr << "Failed to open mesh file: " << fileName << "\n";
    return;
  }
  std::string id;
  size_t nn = 0, ne = 0;
  f >> id >> gridDelta >> id >> nn >> id >> ne;
  nodes.resize(nn);
  for (auto &p : nodes)
    f >> id >> p[0] >> p[1] >> p[2];
  // like the reference, a file holding fewer elements than declared leaves the rest
  // value-initialised (lineMesh.dat: 130 declared, 129 present -> one zero-length line)
  elements.assign(ne, VectorType<unsigned, D>{});
  for (size_t i = 0; i < ne && (f >> id); ++i) {
    VectorType<unsigned, D> e{};
    for (int j = 0; j < D; ++j)
      f >> e[j];
    if (f)
      elements[i] = e;
  }
}

// rayUtil.hpp:340-351: a flat point cloud in the plane spanned by direction[0] x direction[1] at coordinate 0 of
// direction[2], from -extent to +extent in steps of gridDelta (coordinates by repeated addition, like the reference's
// loops: the float sums are the coordinates), normals along +direction[2]
template <typename NumericType>
void createPlaneGrid(const NumericType gridDelta, const NumericType extent, const std::array<int, 3> direction,
                     std::vector<Vec3D<NumericType>> &points, std::vector<Vec3D<NumericType>> &normals) {
  const int outer = direction[0], inner = direction[1], up = direction[2];
  Vec3D<NumericType> unitNormal{0, 0, 0};
  unitNormal[up] = 1;
  Vec3D<NumericType> cursor{-extent, -extent, -extent};
  cursor[up] = 0;
  points.clear();
  normals.clear();
  while (cursor[outer] <= extent) {
    cursor[inner] = -extent;
    while (cursor[inner] <= extent) {
      points.push_back(cursor);
      cursor[inner] += gridDelta;
    }
    cursor[outer] += gridDelta;
  }
  normals.assign(points.size(), unitNormal);
}

template <typename NumericType, int D = 3, typename FluxType = NumericType>
void writeVTK(const std::string &filename, const std::vector<Vec3D<NumericType>> &points,
              const std::vector<FluxType> &flux) {
  // byte for byte the reference's output (rayUtil.hpp:413-449): each coordinate is followed by a
  // blank, |flux| < 1e-6 prints as 0
  std::ofstream f(filename.c_str());
  f << "# vtk DataFile Version 2.0\n" << D << "D Surface\nASCII\nDATASET UNSTRUCTURED_GRID\n";
  f << "POINTS " << points.size() << " float\n";
  for (auto const &p : points) {
    for (int j = 0; j < 3; j++)
      f << static_cast<float>(p[j]) << " ";
    f << "\n";
  }
  f << "CELLS " << points.size() << " " << points.size() * 2 << "\n";
  for (size_t i = 0; i < points.size(); ++i)
    f << 1 << " " << i << "\n";
  f << "CELL_TYPES " << points.size() << "\n";
  for (size_t i = 0; i < points.size(); ++i)
    f << 1 << "\n";
  f << "CELL_DATA " << flux.size() << "\nSCALARS flux float\nLOOKUP_TABLE default\n";
  for (size_t j = 0; j < flux.size(); ++j)
    f << ((std::abs(flux[j]) < 1e-6) ? 0.0 : flux[j]) << "\n";
}

// rayUtil.hpp:451-555: VTK PolyData (lines for D == 2, polygons for D == 3); the flux goes to the
// points if its length is the point count, else to the cells if it is the element count
template <typename NumericType, int D = 3, typename ResultType = NumericType>
void writeVTP(const std::string &filename, const std::vector<Vec3D<NumericType>> &points,
              const std::vector<VectorType<unsigned, D>> &elements, const std::vector<ResultType> &flux) {
  std::ofstream f(filename.c_str());
  if (!f.is_open())
    return;
  const size_t nPoints = points.size(), nElements = elements.size();
  f << "<?xml version=\"1.0\"?>\n<VTKFile type=\"PolyData\" version=\"0.1\" byte_order=\"LittleEndian\">\n  <PolyData>\n";
  f << "    <Piece NumberOfPoints=\"" << nPoints << "\" NumberOfVerts=\"0\" NumberOfLines=\"" << (D == 2 ? nElements : 0)
    << "\" NumberOfStrips=\"0\" NumberOfPolys=\"" << (D == 2 ? 0 : nElements)
    << "\">\n      <Points>\n        <DataArray type=\"Float32\" NumberOfComponents=\"3\" format=\"ascii\">\n";
  for (auto const &p : points)
    f << static_cast<float>(p[0]) << " " << static_cast<float>(p[1]) << " " << static_cast<float>(p[2]) << "\n";
  f << "        </DataArray>\n      </Points>\n      " << (D == 2 ? "<Lines>" : "<Polys>")
    << "\n        <DataArray type=\"Int32\" Name=\"connectivity\" format=\"ascii\">\n";
  for (auto const &e : elements) {
    for (int j = 0; j < D; ++j)
      f << static_cast<int>(e[j]) << " ";
    f << "\n";
  }
  f << "        </DataArray>\n        <DataArray type=\"Int32\" Name=\"offsets\" format=\"ascii\">\n";
  int offset = 0;
  for (size_t i = 0; i < nElements; ++i) {
    offset += D;
    f << offset << "\n";
  }
  f << "        </DataArray>\n      " << (D == 2 ? "</Lines>" : "</Polys>") << "\n";
  if (flux.size() == nPoints || flux.size() == nElements) {
    const bool point = flux.size() == nPoints;
    f << "      " << (point ? "<PointData" : "<CellData") << " Scalars=\"flux\">\n"
      << "        <DataArray type=\"Float32\" Name=\"flux\" format=\"ascii\">\n";
    for (size_t i = 0; i < flux.size(); ++i)
      f << ((std::abs(flux[i]) < 1e-6) ? 0.0f : static_cast<float>(flux[i])) << "\n";
    f << "        </DataArray>\n      " << (point ? "</PointData>" : "</CellData>") << "\n";
  } else if (!flux.empty()) {
    std::cerr << "writeVTP: flux size does not match points or polys; skipping data\n";
  }
  f << "    </Piece>\n  </PolyData>\n</VTKFile>\n";
}
inline void writeVTP(TriangleMesh const &mesh, const std::string &filename, const std::vector<double> &flux) {
  writeVTP<float, 3>(filename, mesh.nodes, mesh.triangles, flux);
}
} // namespace rayInternal
