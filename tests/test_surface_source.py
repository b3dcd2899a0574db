"""The device-side surface source (vr_set_surface_source; the reference's gpu/raygTrace.hpp:267-297 and
gpu/raygSource.hpp:65-81): rays that start ON the surface points, leave along a cosine distribution about each point's
normal and carry the point's weight.

The contract: global ray idx belongs to point idx // R (R = numRaysFixed if set, else numRaysPerPoint); its engine is
mt19937_64(tea3(idx, rngSeed + runNumber)); the sample takes two outputs, r1 then r2; origin = P + N/|N| * offset;
direction = cosine (power 1) about the normal in a Frisvad basis; from there the ray is what the host-ray path makes of
the same origin, direction, weight and draws = 2.  The reference's OptiX path draws from cuRAND, so there is no reference
bit pattern: the host-ray path and the oracle fed the dumped rays are the yardsticks.

Tolerances: sample components 2e-6 absolute (a dozen float32 roundings of values <= 1; numpy's sin / cos are not
bit-equal to the library's glibc restatement), origins relative to their magnitude; device against device bit for bit;
device against oracle: every counter exact, flux L2 within FLUX_TOL as in test_gpu_parity.py."""
import os
import subprocess

import numpy as np
import pytest

import viennaray_amd as vr
from viennaray_amd import BoundaryCondition as BC, TraceDirection as TD, capi
from oracle import pyoracle as po
from helpers import ROOT, l2_rel, trench2d, trench3d, trench_mesh

FLUX_TOL = 1e-4  # the repository's standing tolerance (tests/test_gpu_parity.py)
INFO_KEYS = ("numRays", "totalRaysTraced", "nonGeometryHits", "geometryHits", "particleHits",
             "boundaryHits", "reflections", "raysTerminated")
OFFSET = 1e-4
AREA = 123.5
SEED = 4711


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_surface_source_is_declared_exported_and_bound():
    txt = open(os.path.join(ROOT, "include", "viennaray_amd.h")).read()
    L = vr.load()
    for name in ("vr_set_surface_source", "vr_debug_surface_source_sample"):
        assert name + "(" in txt, name
        assert hasattr(L, name), name
        assert name in capi.SIGNATURES, name
    for cls in (vr.TraceDisk, vr.TraceTriangle):
        for method in ("setSurfaceSource", "clearSurfaceSource", "debugSurfaceSourceSample"):
            assert callable(getattr(cls, method, None)), (cls.__name__, method)


def test_cpp_facade_has_the_surface_source():
    """Trace::setSurfaceSource / clearSurfaceSource with the reference's names and argument types, on TraceDisk<float, 3>
    and TraceTriangle<float, 3>"""
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include", "viennaray_amd"),
                        "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "aux", "facade_surface_source.cpp")],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def info_dict(t):
    i = t.getRayTraceInfo()
    return {k: int(getattr(i, k)) for k in INFO_KEYS}


def _weights(n, seed=5):
    rng = np.random.default_rng(seed)
    return np.exp(rng.uniform(np.log(0.05), np.log(3.0), size=n)).astype(np.float32)


class Scene:
    """a geometry of the golden data, its own points and normals as source points, and makers of a tracer / an oracle"""

    def __init__(self, kind, bc=BC.REFLECTIVE_BOUNDARY):
        self.kind, self.bc = kind, bc
        if kind == "tri3d":
            self.D = 3
            self.gd, self.v, self.tri = trench_mesh()
            a, b, c = (self.v[self.tri[:, k]].astype(np.float64) for k in range(3))
            self.P = ((a + b + c) / 3.0).astype(np.float32)
            self.N = np.cross(b - a, c - a).astype(np.float32)   # (not unit length: the source normalises)
        else:
            self.D = 2 if kind == "disks2d" else 3
            self.gd, self.P, self.N = trench2d() if self.D == 2 else trench3d()
        self.n = len(self.P)
        self.W = _weights(self.n)

    def tracer(self, sticking, R=None, seed=SEED):
        if self.kind == "tri3d":
            t = vr.TraceTriangle(3)
            t.setGeometry(self.v, self.tri, self.gd)
        else:
            t = vr.TraceDisk(self.D)
            t.setGeometry(self.P, self.N, self.gd)
        t.setBoundaryConditions([self.bc] * self.D)
        if self.D == 2:
            t.setSourceDirection(TD.POS_Y)
        t.setParticleType(vr.DiffuseParticle(sticking, "flux"))
        if R is not None:
            t.setNumberOfRaysPerPoint(R)
        t.setRngSeed(seed)
        return t

    def oracle(self, sticking, seed=SEED):
        o = po.Oracle()
        if self.kind == "tri3d":
            o.set_triangles(self.v, self.tri, self.gd, 3)
        else:
            o.set_disks(self.P, self.N, self.gd, self.D)
        o.set_boundary_conditions([int(self.bc)] * self.D)
        if self.D == 2:
            o.set_source_direction(po.POS_Y)
        o.set_particle(po.DIFFUSE, sticking)
        o.set_rng_seed(seed)
        o.set_lazy_rng(True)
        return o

    def surface(self, t, W=None, N=None):
        t.setSurfaceSource(self.P, self.N if N is None else N, self.W if W is None else W, AREA, OFFSET)

    def dump(self, t, R, seed=SEED + 1, first=0, count=None):
        """every ray of the apply with run number 1 (kernel seed = rngSeed + 1)"""
        idx = np.arange(first, first + (self.n * R if count is None else count), dtype=np.uint64)
        return t.debugSurfaceSourceSample(idx, seed)


def _run(t):
    t.apply()
    return t.getFluxF64(), info_dict(t)


def _ref_sample(P, N, R, idx, seed):
    """the sample of the module docstring in numpy float32"""
    f = np.float32
    j = (idx // R).astype(np.int64)
    raw = np.stack([po.mt64_outputs(po.tea3(int(i), seed), 2) for i in idx])
    r1, r2 = po.uniform_float(raw[:, 0]), po.uniform_float(raw[:, 1])
    n = N[j].astype(f)
    n = n / np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])[:, None]
    org = P[j].astype(f) + n * f(OFFSET)
    cosT = np.sqrt(r2)
    sinT = np.sqrt(np.maximum(f(0), f(1) - cosT * cosT))
    phi = (2.0 * np.pi * r1.astype(np.float64)).astype(f)
    sinP, cosP = np.sin(phi), np.cos(phi)
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    s = np.copysign(f(1), nz)
    a = f(-1) / (s + nz)
    b = nx * ny * a
    t = np.stack([f(1) + s * nx * nx * a, s * b, -s * nx], axis=1)
    b2 = np.stack([b, s + ny * ny * a, -ny], axis=1)
    d = n * cosT[:, None] + t * (cosP * sinT)[:, None] + b2 * (sinP * sinT)[:, None]
    d = d / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[:, None]
    assert org.dtype == f and d.dtype == f
    return org, d, n


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["disks3d", "disks2d", "tri3d"])
def test_sample_contract(kind):
    S = Scene(kind)
    R = 7
    t = S.tracer(0.5, R)
    S.surface(t)
    total = S.n * R
    rng = np.random.default_rng(11)
    idx = np.unique(np.concatenate([rng.integers(0, total, size=4000), [0, R - 1, R, total - 1]])).astype(np.uint64)
    org, d, w, k = t.debugSurfaceSourceSample(idx, SEED + 1)
    assert (k == 2).all()
    assert (w.view(np.uint32) == S.W[(idx // R).astype(np.int64)].view(np.uint32)).all()
    rorg, rd, rn = _ref_sample(S.P, S.N, R, idx, SEED + 1)
    scale = np.maximum(1.0, np.abs(rorg).max())
    print(kind, "max |org - ref| / scale", np.abs(org - rorg).max() / scale, "max |dir - ref|", np.abs(d - rd).max())
    assert np.abs(org - rorg).max() <= 2e-6 * scale
    assert np.abs(d - rd).max() <= 2e-6
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1.0).max() <= 1e-6
    assert ((d.astype(np.float64) * rn).sum(axis=1) >= -1e-6).all()
    # normals of another length give the same samples
    for factor in (0.3, 7.0):
        S.surface(t, N=(S.N * np.float32(factor)).astype(np.float32))
        o2, d2, w2, k2 = t.debugSurfaceSourceSample(idx, SEED + 1)
        assert np.abs(o2 - rorg).max() <= 2e-6 * scale and np.abs(d2 - rd).max() <= 2e-6, factor
        assert (w2 == w).all() and (k2 == 2).all()


@pytest.mark.gpu
def test_sample_follows_the_cosine_law():
    S = Scene("disks3d")
    R = 5
    t = S.tracer(0.5, R)
    S.surface(t)
    total = S.n * R
    assert total >= 100_000
    idx = np.arange(total, dtype=np.uint64)
    org, d, w, k = t.debugSurfaceSourceSample(idx, 99)
    n = S.N[(idx // R).astype(np.int64)].astype(np.float64)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    cos = (d.astype(np.float64) * n).sum(axis=1)
    print("mean cos", cos.mean(), "min", cos.min(), "samples", total)
    assert (cos >= -1e-6).all()
    assert abs(cos.mean() - 2.0 / 3.0) <= 0.005   # (standard error at 1e5 samples: 7.5e-4)
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1.0).max() <= 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("bc", [BC.REFLECTIVE_BOUNDARY, BC.PERIODIC_BOUNDARY])
@pytest.mark.parametrize("kind,sticking", [("disks3d", 0.2), ("disks3d", 1.0), ("disks2d", 0.3), ("tri3d", 0.5)])
def test_equivalent_to_the_host_ray_path_and_the_oracle(kind, sticking, bc):
    """the main acceptance test: the surface source against the same rays handed over through setHostRays (bit for bit)
    and traced by the oracle (counters exact, flux within FLUX_TOL)"""
    S = Scene(kind, bc)
    R = 40 if kind == "disks2d" else 6
    t = S.tracer(sticking, R)
    S.surface(t)
    flux, info = _run(t)
    assert t.traceMode() not in (1, 2)        # weighted rays never run an absorbing kernel
    assert info["numRays"] == S.n * R
    org, d, w, k = S.dump(t, R)
    h = S.tracer(sticking, R)
    h.setHostRays(org, d, k, weights=w, sourceArea=AREA)
    hflux, hinfo = _run(h)
    assert hinfo == info
    assert (hflux == flux).all(), l2_rel(flux, hflux)
    assert h.traceMode() == t.traceMode()
    o = S.oracle(sticking)
    o.set_host_rays(org, d, weights=w, source_area=AREA)
    o.set_host_ray_draws(k)
    o.apply(po.max_threads())
    oi = o.info()
    for key in INFO_KEYS:
        assert info[key] == oi[key], (key, info[key], oi[key])
    f32 = t.getLocalData().getVectorData(0)
    err = l2_rel(f32, o.flux())
    print(kind, sticking, int(bc), "flux L2 against the oracle", err, info)
    assert err <= FLUX_TOL, err
    assert l2_rel(t.normalizeFlux(f32), o.normalize_flux(o.flux())) <= FLUX_TOL


@pytest.mark.gpu
def test_rays_leave_a_plane_into_the_open_half_space():
    pts, nrm = vr.io.plane_grid(40, 1.0)
    t = vr.TraceDisk(3)
    t.setGeometry(pts, nrm, 1.0)
    t.setParticleType(vr.DiffuseParticle(0.5, "flux"))
    t.setNumberOfRaysPerPoint(50)
    t.setRngSeed(3)
    t.setSurfaceSource(pts, nrm, _weights(len(pts)), AREA, OFFSET)
    flux, info = _run(t)
    print(info)
    assert info["numRays"] == len(pts) * 50
    assert info["geometryHits"] == 0 and (flux == 0).all()
    assert info["nonGeometryHits"] + info["raysTerminated"] == info["numRays"]


@pytest.mark.gpu
def test_flux_of_an_absorbing_trench_is_bounded_by_the_emitted_weight():
    S = Scene("tri3d")
    R = 10
    t = S.tracer(1.0, R)
    S.surface(t)
    flux, info = _run(t)
    total = float(flux.sum())
    print("sum of raw flux", total, "emitted", R * float(S.W.astype(np.float64).sum()))
    assert 0.0 < total <= R * float(S.W.astype(np.float64).sum()) * (1 + 1e-6)


@pytest.mark.gpu
def test_ray_count_and_index_mapping():
    S = Scene("disks3d")
    t = S.tracer(1.0, 3)
    S.surface(t)
    assert _run(t)[1]["numRays"] == S.n * 3
    t.setNumberOfRaysFixed(5)                  # the reference's rule: the fixed count is the rays PER POINT
    assert _run(t)[1]["numRays"] == S.n * 5
    # all weight on one point: the flux of that point's R rays alone (sticking 1: a ray ends at its first hit, so the
    # ray index, which only seeds the draws after the source sample, does not matter)
    R, j0 = 64, S.n // 3
    t = S.tracer(1.0, R)
    W = np.zeros(S.n, dtype=np.float32)
    W[j0] = S.W[j0]
    S.surface(t, W=W)
    flux, info = _run(t)
    org, d, w, k = S.dump(t, R, first=j0 * R, count=R)
    assert (w == S.W[j0]).all()
    h = S.tracer(1.0, R)
    h.setHostRays(org, d, k, weights=w)
    hflux, hinfo = _run(h)
    assert hflux.sum() > 0 and (hflux == flux).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["disks3d", "tri3d"])
def test_normalisation_uses_the_source_area(kind):
    S = Scene(kind)
    R = 4
    t = S.tracer(0.5, R)
    t.applyPrepare()
    bbox_area = t.getSourceArea()
    assert abs(bbox_area - AREA) > 1.0
    S.surface(t)
    t.apply()
    assert abs(t.getSourceArea() - AREA) <= 1e-4 * AREA
    raw = t.getLocalData().getVectorData(0)
    got, fused = t.normalizeFlux(raw), t.getFluxNormalized()
    org, d, w, k = S.dump(t, R)       # (prepares the next apply: the result above is read first)
    o = S.oracle(0.5)
    o.set_host_rays(org, d, weights=w, source_area=AREA)
    o.set_host_ray_draws(k)
    o.apply(po.max_threads())
    want = o.normalize_flux(raw)
    assert np.nanmax(np.abs(want)) > 0
    assert np.allclose(got, want, rtol=1e-6, atol=0, equal_nan=True)
    assert ((fused.view(np.uint32) == got.view(np.uint32)) | (np.isnan(fused) & np.isnan(got))).all()
    t.clearSurfaceSource()
    t.applyPrepare()
    assert t.getSourceArea() == bbox_area


@pytest.mark.gpu
def test_clearing_restores_the_other_sources_exactly():
    S = Scene("disks3d")

    def plain(t):
        t.setNumberOfRaysPerPoint(5)

    def grid(t):
        t.setNumberOfRaysPerPoint(5)
        t.setSource(vr.SourceGrid(S.P[:256] + np.array([0.0, 0.0, 5.0], dtype=np.float32)))

    src = S.tracer(0.3)
    src.setNumberOfRaysFixed(50_000)
    horg, hdir = src.debugSourceSample(np.arange(50_000, dtype=np.uint64), SEED + 1)

    def host(t):
        t.setHostRays(horg, hdir, np.full(50_000, 4, dtype=np.uint32))

    for name, other in (("plain", plain), ("grid", grid), ("host", host)):
        fresh = S.tracer(0.3)
        other(fresh)
        want = _run(fresh)
        t = S.tracer(0.3)
        S.surface(t)
        if name == "plain":
            t.clearSurfaceSource()
        other(t)
        got = _run(t)
        assert got[1] == want[1], name
        assert (got[0] == want[0]).all(), name
        assert t.getSourceArea() == fresh.getSourceArea(), name
    # ... also after an apply WITH the surface source, and through resetSource()
    t = S.tracer(0.3, 5)
    S.surface(t)
    t.apply()
    t.resetSource()
    t.setRunNumber(1)
    fresh = S.tracer(0.3, 5)
    want, got = _run(fresh), _run(t)
    assert got[1] == want[1] and (got[0] == want[0]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["disks3d", "tri3d"])
def test_ray_range_shards_sum_to_the_whole(kind):
    S = Scene(kind)
    R = 10

    def run(first, count):
        t = S.tracer(0.3, R)
        S.surface(t)
        t.setRayRange(first, count)
        return _run(t)

    total = S.n * R
    whole, wi = run(0, 0)
    assert wi["numRays"] == total
    half = total // 2
    for cuts in ([0, half, total], [0, 3 * R + 3, (2 * S.n // 3) * R + 7, total]):   # (boundaries inside a point's R rays)
        parts = [run(a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
        assert (sum(p[0] for p in parts) == whole).all(), cuts
        for key in INFO_KEYS[1:]:
            assert sum(p[1][key] for p in parts) == wi[key], (cuts, key)


@pytest.mark.gpu
def test_several_particles_share_the_surface_source():
    S = Scene("disks3d")
    R = 5
    t = S.tracer(0.2, R)
    S.surface(t)
    t.setParticleTypes([vr.DiffuseParticle(0.2, "a"), vr.DiffuseParticle(0.7, "b")])
    t.apply()
    assert t.numData() == 2 and t.getRunNumber() == 2
    both = [t.getLocalData().getVectorData(k).copy() for k in range(2)]
    infos = [{k: int(getattr(t.getParticleTraceInfo(q), k)) for k in INFO_KEYS} for q in range(2)]
    for q, sticking in enumerate((0.2, 0.7)):
        s = S.tracer(sticking, R)
        S.surface(s)
        s.apply()
        assert (s.getLocalData().getVectorData(0) == both[q]).all(), q
        assert info_dict(s) == infos[q], q


# a stateful wrapper of the diffuse model (the shape of tests/test_stateful_models.py: INERT)
STATEFUL = """
struct VrUserModel : ModelDiffuse {
  static constexpr bool kNeedsFull = true;
  static constexpr int kStateWords = 1;
  __device__ static void init(const ModelCtx &, RayState &s, Rng &, unsigned &) { s.v[0] = 0.f; }
  template <int D>
  __device__ static Reflection surface_reflection(const ModelCtx &m, RayState &, float w, const V3 &rayDir, const V3 &n,
                                                  unsigned primID, int, float base, Rng &rng, unsigned &t2) {
    Reflection r{ModelDiffuse::sticking(m, primID, base), rayDir};
    if (w - w * r.sticking > 0.f)
      r.dir = ModelDiffuse::reflect<D>(m, rayDir, n, rng, t2);
    return r;
  }
  template <class Credit>
  __device__ static void collide(const ModelCtx &m, const RayState &, float w, const V3 &d, const V3 &n, unsigned primID,
                                 int, Credit &&credit) {
    ModelDiffuse::collide(m, w, d, n, primID, credit);
  }
};
"""


@pytest.mark.gpu
def test_refusals(tmp_path, monkeypatch):
    S = Scene("disks3d")
    R = 3
    t = S.tracer(0.5, R)
    S.surface(t)
    want = _run(t)
    t.setRunNumber(1)
    L, h = t._L, t._h
    fp = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32).ctypes.data_as(capi.C.POINTER(capi.C.c_float))

    def refused(P=S.P, N=S.N, W=S.W, area=1.0, offset=0.0, what=""):
        keep = [np.ascontiguousarray(x, dtype=np.float32) if x is not None else None for x in (P, N, W)]
        rc = L.vr_set_surface_source(h, fp(keep[0]), fp(keep[1]), fp(keep[2]), S.n, area, offset)
        assert rc == capi.VR_E_INVALID, (what, rc)
        assert len(L.vr_last_error(h)) > 0, what

    def changed(a, j, value):
        b = np.array(a, dtype=np.float32, copy=True)
        b[j] = value
        return b

    refused(P=None, what="null positions")
    refused(N=None, what="null normals")
    refused(W=None, what="null weights")
    refused(N=changed(S.N, 17, [0, 0, 0]), what="zero-length normal")
    refused(N=changed(S.N, 17, [np.nan, 0, 1]), what="NaN normal")
    refused(N=changed(S.N, 17, [np.inf, 0, 1]), what="infinite normal")
    refused(W=changed(S.W, 5, -0.5), what="negative weight")
    refused(W=changed(S.W, 5, np.inf), what="infinite weight")
    refused(W=changed(S.W, 5, np.nan), what="NaN weight")
    refused(area=0.0, what="zero area")
    refused(area=-2.0, what="negative area")
    refused(offset=-1e-3, what="negative offset")
    refused(offset=float("nan"), what="NaN offset")
    refused(offset=float("inf"), what="infinite offset")
    with pytest.raises(vr.VrError):
        t.setSurfaceSource(S.P, S.N[:-1], S.W, AREA, OFFSET)
    # the previous source is still in place
    got = _run(t)
    assert got[1] == want[1] and (got[0] == want[0]).all()
    assert abs(t.getSourceArea() - AREA) <= 1e-4 * AREA
    # a stateful run-time model is refused at apply time, as with SourceGrid and host rays
    monkeypatch.setenv("VR_CACHE_DIR", str(tmp_path))
    k = t.registerParticleModel(STATEFUL, numData=1, name="inertDiffuse", numState=1)
    t.setParticleType(vr.UserModelParticle(k, 0.4, ["flux"]))
    with pytest.raises(vr.VrError, match="SourceRandom only"):
        t.apply()
