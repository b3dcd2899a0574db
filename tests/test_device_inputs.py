"""Device-resident inputs of a time step: global data (vr_set_global_data_device), material ids
(vr_set_material_ids_device) and the surface-source tables (vr_set_surface_source_device), and the torch-tensor forms of
Trace.setGlobalData / setGlobalVector / setMaterialIds / setSurfaceSource.

The yardstick is the host entry point with the same values.  A device copy cannot change a bit: everything below compares
flux bits and every TraceInfo counter with `==`, there is no tolerance anywhere."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import viennaray_amd as vr
from viennaray_amd import capi
from helpers import ROOT, trench2d, trench3d, sphere3d, trench_mesh

PER = vr.BoundaryCondition.PERIODIC_BOUNDARY
REF = vr.BoundaryCondition.REFLECTIVE_BOUNDARY
INFO_KEYS = ("numRays", "totalRaysTraced", "nonGeometryHits", "geometryHits", "particleHits", "boundaryHits",
             "reflections", "raysTerminated", "warning", "error", "rngFullStates", "bvhRefits")
FACADE_FLAGS = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include",
                "-I", os.path.join(ROOT, "include", "viennaray_amd"), "-I", os.path.join(ROOT, "include")]
FACADE_SRC = os.path.join(ROOT, "tests", "aux", "facade_device_inputs.cpp")
NEW_SYMBOLS = ("vr_set_global_data_device", "vr_set_material_ids_device", "vr_set_surface_source_device")
AREA, OFFSET = 123.5, 1e-4


# ---------------------------------------------------------------------------------------------------------------------
# no GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_device_input_entry_points_are_declared_exported_and_bound():
    txt = open(os.path.join(ROOT, "include", "viennaray_amd.h")).read()
    L = vr.load()
    for name in NEW_SYMBOLS:
        assert name + "(" in txt, name
        assert hasattr(L, name), name
        assert name in capi.SIGNATURES, name
    assert callable(getattr(vr.Trace, "setGlobalVector", None))


def test_cpp_facade_names_the_device_input_methods():
    hdr = open(os.path.join(ROOT, "include", "viennaray_amd", "viennaray.hpp")).read()
    assert "void setGlobalDataDevice(unsigned vecIdx, const float *dData, size_t n, void *stream" in hdr
    assert "void setMaterialIdsDevice(const int32_t *dIds, size_t n, void *stream" in hdr
    assert "void setSurfaceSourceDevice(const float *dPositions, const float *dNormals, const float *dWeights, size_t n, unsigned ld" in hdr
    p = subprocess.run(["g++", "-fsyntax-only"] + FACADE_FLAGS + [FACADE_SRC], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]


def test_trace_module_still_does_not_import_torch():
    src = open(os.path.join(ROOT, "viennaray_amd", "trace.py")).read()
    for line in src.splitlines():
        assert not line.startswith(("import torch", "from torch")), line


# ---------------------------------------------------------------------------------------------------------------------
# GPU: helpers
# ---------------------------------------------------------------------------------------------------------------------
def _torch():
    import torch
    return torch


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def model_cache(tmp_path_factory):
    """one code-object cache for the module: each run-time model is compiled once"""
    return str(tmp_path_factory.mktemp("vr_inputs_cache"))


# two labels; sticking falls with vector params[0], label 1 is weighted by vector params[1]
TWO_VECTORS = """
struct VrUserModel : ModelDiffuse {
  static constexpr int kNumData = 2;
  __device__ static float sticking(const ModelCtx &m, unsigned primID, float base) {
    return base * (1.f - m.global.vector((unsigned)m.params[0], primID));
  }
  template <class Credit>
  __device__ static void collide(const ModelCtx &m, float w, const V3 &, const V3 &, unsigned primID, Credit &&credit) {
    credit(0, w);
    credit(1, w * m.global.vector((unsigned)m.params[1], primID));
  }
};
"""

# the ion of INTEGRATION.md 3.1, shortened: energy state, sticks where the material says so, credits by material id
ION = """
struct VrUserModel : ModelDiffuse {
  static constexpr int kNumData = 2;
  static constexpr bool kNeedsFull = true;
  static constexpr int kStateWords = 1;
  __device__ static void init(const ModelCtx &m, RayState &s, Rng &, unsigned &) { s.v[0] = m.params[0]; }
  template <int D>
  __device__ static Reflection surface_reflection(const ModelCtx &, RayState &s, float w, const V3 &rayDir, const V3 &n,
                                                  unsigned, int materialId, float base, Rng &rng, unsigned &t2) {
    s.v[0] *= 0.5f;
    Reflection r{materialId == 2 ? 1.f : base, rayDir};
    if (w - w * r.sticking > 0.f)
      r.dir = reflection_diffuse<D>(n, rng, t2);
    return r;
  }
  template <class Credit>
  __device__ static void collide(const ModelCtx &, const RayState &s, float w, const V3 &, const V3 &, unsigned,
                                 int materialId, Credit &&credit) {
    credit(0, w);
    credit(1, materialId == 1 ? w * s.v[0] : 0.f);
  }
};
"""


def _geometry(geom):
    """(D, set-geometry function, primitives)"""
    if geom == "tri3d":
        gd, v, tri = trench_mesh()
        return 3, (lambda t: t.setGeometry(v, tri, gd)), len(tri)
    gd, p, n = {"disks3d": trench3d, "disks2d": trench2d, "sphere3d": sphere3d}[geom]()
    return (2 if geom == "disks2d" else 3), (lambda t: t.setGeometry(p, n, gd)), len(p)


def _tracer(geom, rays=60_000, bc=PER, geometry=True):
    D, setg, n = _geometry(geom)
    t = vr.TraceTriangle(3) if geom == "tri3d" else vr.TraceDisk(D)
    if geometry:
        setg(t)
    t.setBoundaryConditions([bc] * D)
    if D == 2:
        t.setSourceDirection(vr.TraceDirection.POS_Y)
    t.setNumberOfRaysFixed(rays)
    t.setUseRandomSeeds(False)
    t.setRngSeed(4711)
    return t, n


def _run(t):
    """apply with run number 1: (bits of every flux label, counters)"""
    t.setRunNumber(1)
    t.apply()
    i = t.getRayTraceInfo()
    ld = t.getLocalData()
    return ([ld.getVectorData(k).copy().view(np.uint32) for k in range(t.numData())],
            {k: int(getattr(i, k)) for k in INFO_KEYS})


def _same(a, b, what=""):
    assert a[1] == b[1], (what, a[1], b[1])
    assert len(a[0]) == len(b[0]), what
    for k, (x, y) in enumerate(zip(a[0], b[0])):
        assert np.array_equal(x, y), (what, k, int((x != y).sum()))


def _vectors(n, count, seed=3):
    rng = np.random.default_rng(seed)
    return [rng.uniform(0.05, 0.95, n).astype(np.float32) for _ in range(count)]


def _global_particle(t, kind, cache, monkeypatch, params=(0.0, 1.0)):
    if kind == "coverage":
        return vr.CoverageStickingParticle(0.6, "flux", coverageVector=int(params[0]))
    monkeypatch.setenv("VR_CACHE_DIR", cache)
    k = t.registerParticleModel(TWO_VECTORS, numData=2, name="twoVectors")
    return vr.UserModelParticle(k, 0.6, ["flux", "weighted"], params=list(params))


def _pair(geom, kind, cache, monkeypatch, params=(0.0, 1.0), rays=60_000):
    """a tracer for the host way and one for the device way, same scene and particle"""
    out = []
    for _ in range(2):
        t, n = _tracer(geom, rays)
        t.setParticleType(_global_particle(t, kind, cache, monkeypatch, params))
        out.append(t)
    return out[0], out[1], n


# ---------------------------------------------------------------------------------------------------------------------
# GPU: global data
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["coverage", "model"])
@pytest.mark.parametrize("geom", ["disks3d", "disks2d", "tri3d"])
def test_tensor_vectors_equal_numpy_vectors(geom, kind, model_cache, monkeypatch):
    """vector lengths numPrims, numPrims - 1, 1 and numPrims + 7 (longer than the geometry), one after the other on the
    same two contexts: the stride shrinks and grows on the host side, only grows on the device side, the flux is the same"""
    host, dev, n = _pair(geom, kind, model_cache, monkeypatch)
    seen = set()
    for length in (n, n - 1, 1, n + 7):
        vecs = _vectors(length, 2, seed=length)
        host.setGlobalData(vecs)
        tens = [_dev(v) for v in vecs]
        dev.setGlobalData(tens)
        assert dev.getGlobalData() is tens
        a, b = _run(host), _run(dev)
        _same(a, b, (geom, kind, length))
        assert a[1]["error"] == 0 and a[0][0].any()
        seen.add(a[0][0].tobytes())
    assert len(seen) == 4  # (the vectors matter)


@pytest.mark.gpu
def test_a_vector_that_was_never_set_reads_zero(model_cache, monkeypatch):
    """index 2 set, index 1 never: vector 1 reads 0 (label 1 of the model is 0 everywhere), like on the host"""
    host, dev, n = _pair("disks3d", "model", model_cache, monkeypatch, params=(2.0, 1.0))
    v = _vectors(n, 1)[0]
    host.setGlobalVector(2, v)
    dev.setGlobalVector(2, _dev(v))
    a, b = _run(host), _run(dev)
    _same(a, b)
    assert not b[0][1].any() and b[0][0].any()
    plain, _, _ = _pair("disks3d", "model", model_cache, monkeypatch, params=(2.0, 1.0))
    assert not np.array_equal(_run(plain)[0][0], b[0][0])  # (vector 2 was read)


@pytest.mark.gpu
def test_a_longer_vector_re_lays_the_rows_and_keeps_the_others(model_cache, monkeypatch):
    host, dev, n = _pair("disks3d", "model", model_cache, monkeypatch)
    short, other, longer = _vectors(n // 3, 1, 1)[0], _vectors(n // 2, 1, 2)[0], _vectors(n + 7, 1, 3)[0]
    for t, f in ((host, lambda x: x), (dev, _dev)):
        t.setGlobalVector(0, f(short))
        t.setGlobalVector(1, f(other))
    first = _run(host), _run(dev)
    _same(*first, "before the growth")
    for t, f in ((host, lambda x: x), (dev, _dev)):
        t.setGlobalVector(0, f(longer))  # the stride grows from n // 2 to n + 7 with vector 1 in place
    second = _run(host), _run(dev)
    _same(*second, "after the growth")
    assert second[1][0][1].any() and not np.array_equal(first[1][0][0], second[1][0][0])


@pytest.mark.gpu
def test_dropping_from_the_middle_drops_the_vectors_behind(model_cache, monkeypatch):
    host, dev, n = _pair("disks3d", "model", model_cache, monkeypatch, params=(0.0, 2.0))
    vecs = _vectors(n, 3)
    host.setGlobalData(vecs)
    dev.setGlobalData([_dev(v) for v in vecs])
    with_all = _run(dev)
    _same(_run(host), with_all)
    assert with_all[0][1].any()
    L = capi.load()
    host.setGlobalVector(1, None)
    assert L.vr_set_global_data_device(dev._h, 1, None, 0, None) == capi.VR_OK  # n == 0 at index 1: vector 2 goes too
    a, b = _run(host), _run(dev)
    _same(a, b)
    assert not b[0][1].any() and np.array_equal(b[0][0], with_all[0][0])  # vector 0 stayed, vector 2 reads 0
    # ... and an index that comes back reads its new values, the one in between 0
    host.setGlobalVector(2, vecs[1])
    dev.setGlobalVector(2, _dev(vecs[1]))
    a, b = _run(host), _run(dev)
    _same(a, b)
    assert b[0][1].any()


@pytest.mark.gpu
def test_the_seventeenth_vector_is_refused(model_cache, monkeypatch):
    torch = _torch()
    L = capi.load()
    host, dev, n = _pair("disks3d", "coverage", model_cache, monkeypatch)
    v = _vectors(n, 1)[0]
    tv = _dev(v)
    host.setGlobalData([v])
    dev.setGlobalData([tv])
    assert L.vr_set_global_data_device(dev._h, 16, C.c_void_p(tv.data_ptr()), n, None) == capi.VR_E_INVALID
    assert b"at most 16" in L.vr_last_error(dev._h)
    assert L.vr_set_global_data_device(dev._h, 0, v.ctypes.data, n, None) == capi.VR_E_INVALID  # a host pointer
    assert b"not device memory" in L.vr_last_error(dev._h)
    with pytest.raises(ValueError, match="dtype"):
        dev.setGlobalData([tv.double()])
    with pytest.raises(ValueError, match="contiguity"):
        dev.setGlobalData([torch.zeros(n, 2, device="cuda")[:, 0]])
    with pytest.raises(ValueError, match="shape"):
        dev.setGlobalData([torch.zeros(n, 1, device="cuda")])
    _same(_run(host), _run(dev))  # every refusal left the vector in force
    for k in range(16):
        dev.setGlobalVector(k, tv)
    _same(_run(host), _run(dev))


@pytest.mark.gpu
def test_host_and_device_vectors_mix_on_one_context(model_cache, monkeypatch):
    host, dev, n = _pair("disks3d", "model", model_cache, monkeypatch)
    a0, a1, b0, b1 = _vectors(n, 4)
    host.setGlobalData([a0, a1])
    dev.setGlobalData([a0, _dev(a1)])  # vector 0 from the host, vector 1 from a tensor
    _same(_run(host), _run(dev), "host, tensor")
    host.setGlobalData([b0, b1])
    dev.setGlobalData([_dev(b0), b1])  # ... the other way round on the same context
    _same(_run(host), _run(dev), "tensor, host")
    host.setGlobalVector(1, a1)
    dev.setGlobalVector(1, _dev(a1))   # both from tensors now
    _same(_run(host), _run(dev), "tensor, tensor")
    host.setGlobalVector(0, a0)
    dev.setGlobalVector(0, a0)         # a host vector over a device-set one
    _same(_run(host), _run(dev), "host over tensor")


@pytest.mark.gpu
def test_the_vector_is_copied_when_it_is_set(model_cache, monkeypatch):
    host, dev, n = _pair("disks3d", "coverage", model_cache, monkeypatch)
    v = _vectors(n, 1)[0]
    host.setGlobalData([v])
    tv = _dev(v)
    dev.setGlobalData([tv])
    tv.zero_()  # on the same stream, right behind the call
    _same(_run(host), _run(dev))


@pytest.mark.gpu
def test_a_vector_produced_on_a_side_stream_needs_no_synchronize(model_cache, monkeypatch):
    torch = _torch()
    host, dev, n = _pair("disks3d", "coverage", model_cache, monkeypatch)
    v = _vectors(n, 1)[0]
    host.setGlobalData([v])
    hv = _dev(v)
    a = torch.randn(3072, 3072, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        m = a
        for _ in range(4):
            m = (m @ a) * 1e-3
        keep = (m[0, 0] * 0.0).nan_to_num(0.0)  # (0, but only once the matmuls are through)
        tv = hv + keep
        dev.setGlobalData([tv])
        tv.zero_()
    _same(_run(host), _run(dev))
    s.synchronize()


@pytest.mark.gpu
def test_a_coverage_loop_with_torch_ops_only(model_cache, monkeypatch):
    """ten iterations of trace -> coverage = f(flux) -> trace: through tensors (getFluxTensor, torch ops, setGlobalVector)
    and through numpy; f uses exactly rounded float32 operations only, so both ways compute the same coverages"""
    torch = _torch()
    host, dev, n = _pair("disks3d", "coverage", model_cache, monkeypatch, rays=30_000)
    f = np.float32
    cov_h = np.zeros(n, dtype=f)
    cov_d = torch.zeros(n, dtype=torch.float32, device="cuda")
    for _ in range(10):
        host.setGlobalVector(0, cov_h)
        dev.setGlobalVector(0, cov_d)
        host.setRunNumber(1)
        dev.setRunNumber(1)
        host.apply()
        dev.apply(collect=False)
        flux_h = host.getLocalData().getVectorData(0)
        flux_d = dev.getFluxTensor()
        cov_h = cov_h * f(0.5) + np.minimum(flux_h * f(0.03125), f(1.0)) * f(0.5)
        cov_d = cov_d * 0.5 + torch.clamp(flux_d * 0.03125, max=1.0) * 0.5
    assert np.array_equal(flux_d.cpu().numpy().view(np.uint32), flux_h.view(np.uint32))
    assert np.array_equal(cov_d.cpu().numpy().view(np.uint32), cov_h.view(np.uint32))
    assert cov_h.max() > 0.1


# ---------------------------------------------------------------------------------------------------------------------
# GPU: material ids
# ---------------------------------------------------------------------------------------------------------------------
class _Pairs(list):
    """a materialSticking "map" that may hold an id twice (the C ABI takes a list of pairs; the last one wins)"""

    def keys(self):
        return [k for k, _ in self]

    def values(self):
        return [v for _, v in self]


def _material_particle(pairs=((0, 0.2), (1, 0.7), (2, 0.4), (1, 0.05)), base=0.9):
    p = vr.DiffuseParticle(base, "flux")
    p.materialSticking = _Pairs(pairs)  # ids 0, 1, 2 with 1 given twice; id 3 of the geometry is not in the map
    return p


def _ids(n, seed=11):
    return np.random.default_rng(seed).integers(0, 4, n).astype(np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("geom", ["disks3d", "tri3d"])
def test_material_sticking_from_a_tensor(geom):
    ref, n = _tracer(geom)
    ref.setParticleType(vr.DiffuseParticle(0.9, "flux"))
    plain = _run(ref)
    ids = _ids(n)
    seen = []
    for count in (n, n // 2):  # (fewer ids than primitives: the tail has id 0)
        host, _ = _tracer(geom)
        dev, _ = _tracer(geom)
        for t in (host, dev):
            t.setParticleType(_material_particle())
        host.setMaterialIds(ids[:count])
        dev.setMaterialIds(_dev(ids[:count]))
        a, b = _run(host), _run(dev)
        _same(a, b, (geom, count))
        seen.append(b[0][0].tobytes())
        # the duplicated id takes its LAST value: the same map without the first entry of id 1
        last, _ = _tracer(geom)
        last.setParticleType(_material_particle(((0, 0.2), (2, 0.4), (1, 0.05))))
        last.setMaterialIds(ids[:count])
        _same(_run(last), b, "last match wins")
    assert seen[0] != seen[1] and plain[0][0].tobytes() not in seen


@pytest.mark.gpu
@pytest.mark.parametrize("geom", ["disks3d", "tri3d"])
def test_material_ids_reach_a_stateful_model_from_a_tensor(geom, model_cache, monkeypatch):
    monkeypatch.setenv("VR_CACHE_DIR", model_cache)
    _, _, n = _geometry(geom)
    ids = _ids(n)
    for count in (n, n - 5):
        res = []
        for way in ("host", "device"):
            t, _ = _tracer(geom)
            k = t.registerParticleModel(ION, numData=2, name="ion", numState=1)
            t.setParticleType(vr.UserModelParticle(k, 0.3, ["all", "mat1"], params=[8.0]))
            t.setMaterialIds(ids[:count] if way == "host" else _dev(ids[:count]))
            res.append(_run(t))
        _same(res[0], res[1], (geom, count))
        mat1 = res[1][0][1].view(np.float32)
        assert mat1.any() and not mat1[np.r_[ids[:count], np.zeros(n - count, np.int32)] != 1].any()


@pytest.mark.gpu
def test_two_particles_with_different_maps():
    host, n = _tracer("disks3d")
    dev, _ = _tracer("disks3d")
    ids = _ids(n)
    for t in (host, dev):
        t.setParticleTypes([_material_particle(), _material_particle(((3, 0.1), (0, 1.0)), base=0.5)])
    host.setMaterialIds(ids)
    dev.setMaterialIds(_dev(ids))
    a, b = _run(host), _run(dev)
    _same(a, b)
    assert len(b[0]) == 2 and not np.array_equal(b[0][0], b[0][1])
    for q in range(2):
        ia, ib = host.getParticleTraceInfo(q), dev.getParticleTraceInfo(q)
        assert all(int(getattr(ia, k)) == int(getattr(ib, k)) for k in INFO_KEYS), q


@pytest.mark.gpu
def test_ids_before_and_after_the_geometry_and_across_a_geometry_change():
    _, set3d, n = _geometry("disks3d")
    _, sets, ns = _geometry("sphere3d")
    assert n != ns
    ids = _ids(n)
    res = []
    for f in ((lambda x: x), _dev):
        out = []
        t, _ = _tracer("disks3d", geometry=False)
        t.setParticleType(_material_particle())
        t.setMaterialIds(f(ids))  # before the geometry: kept, the primitive count fits
        set3d(t)
        out.append(_run(t))
        t.setMaterialIds(f(ids[::-1].copy()))  # after it
        out.append(_run(t))
        set3d(t)  # the same count again: the ids stay
        out.append(_run(t))
        sets(t)   # another count: every id reads 0
        out.append(_run(t))
        t.setMaterialIds(f(_ids(ns, 5)))
        out.append(_run(t))
        res.append(out)
    for k, (a, b) in enumerate(zip(*res)):
        _same(a, b, k)
    assert np.array_equal(res[1][1][0][0], res[1][2][0][0]) and not np.array_equal(res[1][0][0][0], res[1][1][0][0])
    fresh, _ = _tracer("sphere3d")
    fresh.setParticleType(_material_particle())
    _same(_run(fresh), res[1][3], "ids reset to 0")
    assert not np.array_equal(res[1][3][0][0], res[1][4][0][0])
    L = capi.load()
    assert L.vr_set_material_ids_device(t._h, ids.ctypes.data, n, None) == capi.VR_E_INVALID
    assert b"not device memory" in L.vr_last_error(t._h)
    with pytest.raises(ValueError, match="dtype"):
        t.setMaterialIds(_dev(ids).long())
    _same(_run(t), res[1][4], "refusals keep the ids")


# ---------------------------------------------------------------------------------------------------------------------
# GPU: surface source
# ---------------------------------------------------------------------------------------------------------------------
class Scene:
    """a geometry, its own points and normals as source points (tests/test_surface_source.py: Scene)"""

    def __init__(self, kind, bc=REF):
        self.kind, self.bc = kind, bc
        if kind == "tri3d":
            self.D = 3
            self.gd, self.v, self.tri = trench_mesh()
            a, b, c = (self.v[self.tri[:, k]].astype(np.float64) for k in range(3))
            self.P = ((a + b + c) / 3.0).astype(np.float32)
            self.N = np.cross(b - a, c - a).astype(np.float32)  # (not unit length: the source normalises)
        else:
            self.D = 2 if kind == "disks2d" else 3
            self.gd, self.P, self.N = trench2d() if self.D == 2 else trench3d()
        self.n = len(self.P)
        rng = np.random.default_rng(5)
        self.W = np.exp(rng.uniform(np.log(0.05), np.log(3.0), size=self.n)).astype(np.float32)

    def tracer(self, sticking, R):
        if self.kind == "tri3d":
            t = vr.TraceTriangle(3)
            t.setGeometry(self.v, self.tri, self.gd)
        else:
            t = vr.TraceDisk(self.D)
            t.setGeometry(self.P, self.N, self.gd)
        t.setBoundaryConditions([self.bc] * self.D)
        if self.D == 2:
            t.setSourceDirection(vr.TraceDirection.POS_Y)
        t.setParticleType(vr.DiffuseParticle(sticking, "flux"))
        t.setNumberOfRaysPerPoint(R)
        t.setUseRandomSeeds(False)
        t.setRngSeed(4711)
        return t


def _sample(t, count):
    idx = np.unique(np.linspace(0, count - 1, 257).astype(np.uint64))
    return [x.copy().view(np.uint32) for x in t.debugSurfaceSourceSample(idx, 4712)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,sticking,bc", [("disks3d", 0.2, REF), ("disks3d", 1.0, PER), ("disks2d", 0.3, PER),
                                              ("tri3d", 0.5, REF)])
def test_surface_source_from_tensors(kind, sticking, bc):
    S = Scene(kind, bc)
    R = 40 if kind == "disks2d" else 6
    host, dev = S.tracer(sticking, R), S.tracer(sticking, R)
    host.setSurfaceSource(S.P, S.N, S.W, AREA, OFFSET)
    dev.setSurfaceSource(_dev(S.P), _dev(S.N), _dev(S.W), AREA, OFFSET)
    a, b = _run(host), _run(dev)
    _same(a, b, kind)
    assert a[1]["numRays"] == S.n * R and a[0][0].any()
    assert host.traceMode() == dev.traceMode() and host.getSourceArea() == dev.getSourceArea()
    for x, y in zip(_sample(host, S.n * R), _sample(dev, S.n * R)):  # origins, directions, weights, draws
        assert np.array_equal(x, y)


@pytest.mark.gpu
def test_rows_of_two_floats_on_a_2d_context_only():
    S = Scene("disks2d", PER)
    host, dev = S.tracer(0.3, 40), S.tracer(0.3, 40)
    host.setSurfaceSource(S.P, S.N, S.W, AREA, OFFSET)
    assert not S.P[:, 2].any() and not S.N[:, 2].any()
    dev.setSurfaceSource(_dev(S.P[:, :2]), _dev(S.N[:, :2]), _dev(S.W), AREA, OFFSET)
    _same(_run(host), _run(dev))
    for x, y in zip(_sample(host, S.n * 40), _sample(dev, S.n * 40)):
        assert np.array_equal(x, y)
    S3 = Scene("disks3d")
    t = S3.tracer(0.3, 3)
    t.setSurfaceSource(S3.P, S3.N, S3.W, AREA, OFFSET)
    want = _run(t)
    p2, n2, w = _dev(S3.P[:, :2]), _dev(S3.N[:, :2]), _dev(S3.W)
    with pytest.raises(ValueError, match="shape"):
        t.setSurfaceSource(p2, n2, w, AREA, OFFSET)
    L = capi.load()
    ptr = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    assert L.vr_set_surface_source_device(t._h, ptr(p2), ptr(n2), ptr(w), S3.n, 2, AREA, OFFSET, None) == capi.VR_E_INVALID
    assert b"D == 2" in L.vr_last_error(t._h)
    assert L.vr_set_surface_source_device(t._h, ptr(p2), ptr(n2), ptr(w), S3.n, 4, AREA, OFFSET, None) == capi.VR_E_INVALID
    assert b"2 or 3" in L.vr_last_error(t._h)
    _same(want, _run(t))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_surface_source_sizes(n):
    """the tail of a wave, the tail of a block, more than one block"""
    S = Scene("disks3d")
    R = max(5, 20_000 // n)
    sel = np.linspace(0, S.n - 1, n).astype(np.int64)
    P, N, W = S.P[sel], S.N[sel], S.W[sel]
    host, dev = S.tracer(0.3, R), S.tracer(0.3, R)
    host.setSurfaceSource(P, N, W, AREA, OFFSET)
    dev.setSurfaceSource(_dev(P), _dev(N), _dev(W), AREA, OFFSET)
    a, b = _run(host), _run(dev)
    _same(a, b, n)
    assert a[1]["numRays"] == n * R and a[0][0].any()


@pytest.mark.gpu
def test_weights_computed_from_the_first_pass_on_the_device():
    torch = _torch()
    S = Scene("disks3d", PER)
    f = np.float32
    host, dev = S.tracer(0.3, 8), S.tracer(0.3, 8)
    host.apply()
    dev.apply(collect=False)
    flux_h, flux_d = host.getLocalData().getVectorData(0), dev.getFluxTensor()
    w_h = np.minimum(flux_h * f(0.125), f(2.0)) * f(0.5) + f(0.25)
    w_d = torch.clamp(flux_d * 0.125, max=2.0) * 0.5 + 0.25
    host.setSurfaceSource(S.P, S.N, w_h, AREA, OFFSET)
    dev.setSurfaceSource(_dev(S.P), _dev(S.N), w_d, AREA, OFFSET)
    _same(_run(host), _run(dev))
    assert len(np.unique(w_h)) > 10


def _host_error(t, P, N, W):
    with pytest.raises(vr.VrError) as e:
        t.setSurfaceSource(P, N, W, AREA, OFFSET)
    return str(e.value)


@pytest.mark.gpu
def test_a_refused_surface_source_names_the_hosts_row_and_keeps_the_previous_one():
    S = Scene("disks3d")
    n = 1000
    P, N, W = S.P[:n].copy(), S.N[:n].copy(), S.W[:n].copy()
    host, dev = S.tracer(0.3, 5), S.tracer(0.3, 5)
    host.setSurfaceSource(S.P, S.N, S.W, AREA, OFFSET)
    dev.setSurfaceSource(_dev(S.P), _dev(S.N), _dev(S.W), AREA, OFFSET)
    want = _run(host)

    def changed(a, rows):
        b = a.copy()
        for j, v in rows:
            b[j] = v
        return b

    cases = {
        "NaN position at row 0": (changed(P, [(0, [np.nan, 0, 0])]), N, W, "position 0 is not finite"),
        "zero normal at the last row": (P, changed(N, [(n - 1, [0, 0, 0])]), W, f"normal {n - 1} has zero"),
        "weight 700, position 300": (changed(P, [(300, [0, np.inf, 0])]), N, changed(W, [(700, -0.5)]),
                                     "position 300 is not finite"),
        "one row, position and weight": (changed(P, [(412, [0, 0, -np.inf])]), N, changed(W, [(412, np.nan)]),
                                         "position 412 is not finite"),
        "normal before weight in one row": (P, changed(N, [(9, [np.inf, 0, 0])]), changed(W, [(9, -1.0)]),
                                            "normal 9 has zero or non-finite length"),
        "a weight alone": (P, N, changed(W, [(999, np.inf)]), "weight 999 is negative or not finite"),
    }
    for what, (p, m, w, text) in cases.items():
        msg = _host_error(host, p, m, w)
        assert text in msg, (what, msg)
        with pytest.raises(vr.VrError) as e:
            dev.setSurfaceSource(_dev(p), _dev(m), _dev(w), AREA, OFFSET)
        assert str(e.value) == msg, what
        _same(want, _run(dev), what)  # the previous source, bit for bit
    for area, offset in ((0.0, OFFSET), (AREA, -1.0), (AREA, float("nan"))):
        with pytest.raises(vr.VrError) as eh:
            host.setSurfaceSource(P, N, W, area, offset)
        with pytest.raises(vr.VrError) as ed:
            dev.setSurfaceSource(_dev(P), _dev(N), _dev(W), area, offset)
        assert str(ed.value) == str(eh.value)
    _same(want, _run(dev))


@pytest.mark.gpu
def test_further_surface_source_refusals_leave_the_context_usable(model_cache, monkeypatch):
    torch = _torch()
    L = capi.load()
    S = Scene("disks3d")
    t = S.tracer(0.3, 5)
    tp, tn, tw = _dev(S.P), _dev(S.N), _dev(S.W)
    t.setSurfaceSource(tp, tn, tw, AREA, OFFSET)
    want = _run(t)
    fp = lambda a: a.ctypes.data  # noqa: E731
    assert L.vr_set_surface_source_device(t._h, fp(S.P), fp(S.N), fp(S.W), S.n, 3, AREA, OFFSET, None) == capi.VR_E_INVALID
    assert b"not device memory" in L.vr_last_error(t._h)
    with pytest.raises(ValueError, match="dtype"):
        t.setSurfaceSource(tp.double(), tn.double(), tw.double(), AREA, OFFSET)
    with pytest.raises(ValueError, match="dtype"):
        t.setSurfaceSource(tp, tn, tw.half(), AREA, OFFSET)
    wide = torch.zeros(S.n, 4, device="cuda")
    with pytest.raises(ValueError, match="contiguity"):
        t.setSurfaceSource(wide[:, :3], tn, tw, AREA, OFFSET)
    with pytest.raises(ValueError, match="device"):
        t.setSurfaceSource(tp, tn, S.W, AREA, OFFSET)  # positions on the device, weights on the host
    with pytest.raises(ValueError, match="device"):
        t.setSurfaceSource(tp.cpu(), tn, tw, AREA, OFFSET)
    with pytest.raises(ValueError, match="shape"):
        t.setSurfaceSource(tp, tn, tw[:-1].contiguous(), AREA, OFFSET)
    _same(want, _run(t))
    # a stateful run-time model: refused at apply time with the host setter's message
    monkeypatch.setenv("VR_CACHE_DIR", model_cache)
    k = t.registerParticleModel(ION, numData=2, name="ion", numState=1)
    t.setParticleType(vr.UserModelParticle(k, 0.3, ["all", "mat1"], params=[8.0]))
    with pytest.raises(vr.VrError, match="SourceRandom only"):
        t.apply()
    t.setParticleType(vr.DiffuseParticle(0.3, "flux"))
    _same(want, _run(t))


@pytest.mark.gpu
def test_clearing_after_a_device_set_restores_source_random():
    S = Scene("disks3d")
    fresh = S.tracer(0.3, 5)
    want = _run(fresh)
    for how in ("clearSurfaceSource", "resetSource"):
        t = S.tracer(0.3, 5)
        t.setSurfaceSource(_dev(S.P), _dev(S.N), _dev(S.W), AREA, OFFSET)
        t.apply()
        getattr(t, how)()
        _same(want, _run(t), how)
        assert t.getSourceArea() == fresh.getSourceArea()


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the whole step on the device
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_time_steps_with_tensors_at_every_interface():
    """disks in, coverages in, pass 1, flux out, surface source in (weights from that flux), pass 2, flux out — with
    tensors at every interface against host arrays at every interface"""
    torch = _torch()
    f = np.float32
    gd, p0, n0 = trench3d()
    n = len(p0)
    steps = []
    for k in range(2):  # the surface of step k: the trench shifted a little (another BVH, the same primitive count)
        p = p0.copy()
        p[:, 2] += f(0.125 * k)
        steps.append((p, n0))

    def configure(t):
        t.setBoundaryConditions([PER] * 3)
        t.setUseRandomSeeds(False)
        t.setRngSeed(4711)
        t.setParticleType(vr.CoverageStickingParticle(0.6, "flux"))

    host, dev = vr.TraceDisk(3), vr.TraceDisk(3)
    configure(host)
    configure(dev)
    cov_h = np.full(n, 0.25, dtype=f)
    cov_d = torch.full((n,), 0.25, dtype=torch.float32, device="cuda")
    for k, (p, nrm) in enumerate(steps):
        tp, tn = _dev(p), _dev(nrm)
        host.setGeometry(p, nrm, gd)
        dev.setGeometry(tp, tn, gd)
        host.setGlobalVector(0, cov_h)
        dev.setGlobalVector(0, cov_d)
        for t in (host, dev):
            t.clearSurfaceSource()
            t.setNumberOfRaysFixed(60_000)
            t.setRunNumber(1)
        host.apply()
        dev.apply(collect=False)
        f1_h, f1_d = host.getLocalData().getVectorData(0).copy(), dev.getFluxTensor()
        assert np.array_equal(f1_d.cpu().numpy().view(np.uint32), f1_h.view(np.uint32)), ("pass 1", k)
        i1 = [t.getRayTraceInfo() for t in (host, dev)]
        assert all(int(getattr(i1[0], key)) == int(getattr(i1[1], key)) for key in INFO_KEYS), ("pass 1", k)
        w_h = np.minimum(f1_h * f(0.0625), f(1.0)) * (f(1.0) - cov_h)
        w_d = torch.clamp(f1_d * 0.0625, max=1.0) * (1.0 - cov_d)
        host.setSurfaceSource(p, nrm, w_h, AREA, OFFSET)
        dev.setSurfaceSource(tp, tn, w_d, AREA, OFFSET)
        for t in (host, dev):
            t.setNumberOfRaysPerPoint(8)
            t.setRunNumber(2)
        host.apply()
        dev.apply(collect=False)
        f2_h, f2_d = host.getLocalData().getVectorData(0).copy(), dev.getFluxTensor()
        assert f2_h.any()
        assert np.array_equal(f2_d.cpu().numpy().view(np.uint32), f2_h.view(np.uint32)), ("pass 2", k)
        i2 = [t.getRayTraceInfo() for t in (host, dev)]
        assert all(int(getattr(i2[0], key)) == int(getattr(i2[1], key)) for key in INFO_KEYS), ("pass 2", k)
        cov_h = cov_h * f(0.5) + np.minimum((f1_h + f2_h) * f(0.03125), f(1.0)) * f(0.5)
        cov_d = cov_d * 0.5 + torch.clamp((f1_d + f2_d) * 0.03125, max=1.0) * 0.5
    assert np.array_equal(cov_d.cpu().numpy().view(np.uint32), cov_h.view(np.uint32))


@pytest.mark.gpu
def test_cpp_facade_device_inputs(tmp_path):
    """tests/aux/facade_device_inputs.cpp: the two-pass step through the C++ façade with hipMalloc'd buffers against the
    host setters; a device-set global vector survives apply() calls around a borrowed TracingData"""
    exe = tmp_path / "facade_device_inputs"
    lib = os.path.join(ROOT, "viennaray_amd")
    subprocess.check_call(["g++", "-O1"] + FACADE_FLAGS + [FACADE_SRC, "-o", str(exe), "-L", lib, "-lviennaray_amd",
                                                          "-L", "/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib,
                                                          "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "facade device inputs ok" in out.stdout, out.stdout + out.stderr
