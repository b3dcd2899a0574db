"""Stateful device particle models (vr_particles.hpp, kStateWords > 0; vr_register_particle_model_ex): per-ray state
carried from init (the reference's initNew, rayTraceKernel.hpp:131-133) through every hit, one surface_reflection call per
hit that gives the sticking and the new direction (rayTraceKernel.hpp:310), and the material id of the hit primitive in
both hooks (rayParticle.hpp:21-81).

The oracle has no stateful particles; these tests use what it offers — flux, counters, host rays with draw counts and the
event log (per ray: the primitive and the weight of every surface hit).  Flux against the oracle is compared as in
test_gpu_parity.py: every counter exact, the flux to 5e-6 L2 (float summation order); device against device is bit for bit.
Sums rebuilt from the event log are compared per primitive to 1e-6 relative (the device sums fixed-point weights of the
same float32 values; the rebuild sums them in float64)."""
import os
import subprocess

import numpy as np
import pytest

import viennaray_amd as vr
from viennaray_amd import BoundaryCondition as BC, TraceDirection as TD
from oracle import pyoracle as po
from helpers import l2_rel, trench2d, trench3d, trench_mesh

INFO_KEYS = ("numRays", "totalRaysTraced", "nonGeometryHits", "geometryHits", "particleHits",
             "boundaryHits", "reflections", "raysTerminated")
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "viennaray_amd", "csrc")


def info_dict(t):
    i = t.getRayTraceInfo()
    return {k: int(getattr(i, k)) for k in INFO_KEYS}


# a stateful wrapper of a stateless model: the state is carried but never read, init draws nothing
INERT = """
struct VrUserModel : %(base)s {
  static constexpr bool kNeedsFull = true;
  static constexpr int kStateWords = 1;
  __device__ static void init(const ModelCtx &, RayState &s, Rng &, unsigned &) { s.v[0] = 0.f; }
  template <int D>
  __device__ static Reflection surface_reflection(const ModelCtx &m, RayState &, float w, const V3 &rayDir, const V3 &n,
                                                  unsigned primID, int, float base, Rng &rng, unsigned &t2) {
    Reflection r{%(base)s::sticking(m, primID, base), rayDir};
    if (w - w * r.sticking > 0.f)
      r.dir = %(base)s::reflect<D>(m, rayDir, n, rng, t2);
    return r;
  }
  template <class Credit>
  __device__ static void collide(const ModelCtx &m, const RayState &, float w, const V3 &d, const V3 &n, unsigned primID,
                                 int, Credit &&credit) {
    %(base)s::collide(m, w, d, n, primID, credit);
  }
};
"""

# diffuse; s.v[0] counts the surface hits: label 0 += w, label 1 += w [this is hit 1], label 2 += w * (number of this hit)
HIT_COUNTER = """
struct VrUserModel : ModelDiffuse {
  static constexpr int kNumData = 3;
  static constexpr bool kNeedsFull = true;
  static constexpr int kStateWords = 1;
  __device__ static void init(const ModelCtx &, RayState &s, Rng &, unsigned &) { s.v[0] = 0.f; }
  template <int D>
  __device__ static Reflection surface_reflection(const ModelCtx &, RayState &s, float w, const V3 &rayDir, const V3 &n,
                                                  unsigned, int, float base, Rng &rng, unsigned &t2) {
    s.v[0] += 1.f;
    Reflection r{base, rayDir};
    if (w - w * base > 0.f)
      r.dir = reflection_diffuse<D>(n, rng, t2);
    return r;
  }
  template <class Credit>
  __device__ static void collide(const ModelCtx &, const RayState &s, float w, const V3 &, const V3 &, unsigned, int,
                                 Credit &&credit) {
    const float hit = s.v[0] + 1.f;
    credit(0, w);
    credit(1, hit == 1.f ? w : 0.f);
    credit(2, w * hit);
  }
};
"""

# diffuse whose init draws params[0] engine outputs before the source sample (initNew consuming the engine)
INIT_DRAWS = """
struct VrUserModel : ModelDiffuse {
  static constexpr bool kNeedsFull = true;
  static constexpr int kStateWords = 2;
  __device__ static void init(const ModelCtx &m, RayState &s, Rng &rng, unsigned &t2) {
    s.v[0] = 0.f;
    for (int k = 0; k < (int)m.params[0]; ++k)
      s.v[1] = canon_f32(rng_next(rng, t2));
  }
  template <int D>
  __device__ static Reflection surface_reflection(const ModelCtx &, RayState &, float w, const V3 &rayDir, const V3 &n,
                                                  unsigned, int, float base, Rng &rng, unsigned &t2) {
    Reflection r{base, rayDir};
    if (w - w * base > 0.f)
      r.dir = reflection_diffuse<D>(n, rng, t2);
    return r;
  }
  template <class Credit>
  __device__ static void collide(const ModelCtx &, const RayState &, float w, const V3 &, const V3 &, unsigned, int,
                                 Credit &&credit) {
    credit(0, w);
  }
};
"""

# material ids in both hooks: label 1 += w [material 1]; sticking 1 on material 2, 0 elsewhere (params[0] = 1 switches
# the material sticking on; 0: the particle's own)
MATERIAL = """
struct VrUserModel : ModelDiffuse {
  static constexpr int kNumData = 2;
  static constexpr bool kNeedsFull = true;
  static constexpr int kStateWords = 1;
  __device__ static void init(const ModelCtx &, RayState &s, Rng &, unsigned &) { s.v[0] = 0.f; }
  template <int D>
  __device__ static Reflection surface_reflection(const ModelCtx &m, RayState &, float w, const V3 &rayDir, const V3 &n,
                                                  unsigned, int materialId, float base, Rng &rng, unsigned &t2) {
    Reflection r{m.params[0] > 0.f ? (materialId == 2 ? 1.f : 0.f) : base, rayDir};
    if (w - w * r.sticking > 0.f)
      r.dir = reflection_diffuse<D>(n, rng, t2);
    return r;
  }
  template <class Credit>
  __device__ static void collide(const ModelCtx &, const RayState &, float w, const V3 &, const V3 &, unsigned,
                                 int materialId, Credit &&credit) {
    credit(0, w);
    credit(1, materialId == 1 ? w : 0.f);
  }
};
"""

# energy known answer: init E = params[0] (no draws); every hit halves E, the particle sticks once E < params[1] and
# reflects specularly otherwise.  label 0 += w, label 1 += E at the hit
ENERGY = """
struct VrUserModel : ModelDiffuse {
  static constexpr int kNumData = 2;
  static constexpr bool kNeedsFull = true;
  static constexpr int kStateWords = 1;
  __device__ static void init(const ModelCtx &m, RayState &s, Rng &, unsigned &) { s.v[0] = m.params[0]; }
  template <int D>
  __device__ static Reflection surface_reflection(const ModelCtx &m, RayState &s, float, const V3 &rayDir, const V3 &n,
                                                  unsigned, int, float, Rng &, unsigned &) {
    s.v[0] *= 0.5f;
    return Reflection{s.v[0] < m.params[1] ? 1.f : 0.f, reflect_specular(rayDir, n)};
  }
  template <class Credit>
  __device__ static void collide(const ModelCtx &, const RayState &s, float w, const V3 &, const V3 &, unsigned, int,
                                 Credit &&credit) {
    credit(0, w);
    credit(1, s.v[0]);
  }
};
"""


@pytest.fixture(scope="module")
def model_cache(tmp_path_factory):
    """one code-object cache for the module: each model is compiled once"""
    return str(tmp_path_factory.mktemp("vr_state_cache"))


def _disks(geom):
    gd, p, n = {"trench3d": trench3d, "trench2d": trench2d}[geom]()
    D = 2 if geom == "trench2d" else 3
    t = vr.TraceDisk(D)
    t.setGeometry(p, n, gd)
    o = po.Oracle()
    o.set_disks(p, n, gd, D)
    if D == 2:
        t.setSourceDirection(TD.POS_Y)
        o.set_source_direction(po.POS_Y)
        t.setBoundaryConditions([BC.PERIODIC_BOUNDARY] * 2)
        o.set_boundary_conditions([po.PERIODIC] * 2)
    return t, o, p


def _mesh():
    gd, v, tri = trench_mesh()
    t = vr.TraceTriangle(3)
    t.setGeometry(v, tri, gd)
    o = po.Oracle()
    o.set_triangles(v, tri, gd, 3)
    return t, o, tri


def _scene(geom):
    if geom == "mesh":
        t, o, tri = _mesh()
        return t, o, len(tri)
    t, o, p = _disks(geom)
    return t, o, len(p)


def _rays(t, o, n, seed):
    t.setNumberOfRaysFixed(n)
    o.set_num_rays_fixed(n)
    t.setRngSeed(seed)
    o.set_rng_seed(seed)
    o.set_lazy_rng(True)


def _surface_events(o):
    """kind-3 events (surface hits) of the oracle's log, with the number of each hit along its ray (1, 2, ...)"""
    ev = o.events()
    sel = ev["kind"] == 3
    ray, prim, w = ev["ray"][sel], ev["prim"][sel].astype(np.int64), ev["weight"][sel]
    order = np.argsort(ray, kind="stable")   # (single-threaded log: already in ray order, hits in sequence)
    ray, prim, w = ray[order], prim[order], w[order]
    start = np.r_[True, ray[1:] != ray[:-1]]
    first = np.maximum.accumulate(np.where(start, np.arange(ray.size), 0))
    nth = np.arange(ray.size) - first + 1
    return ray, prim, w, nth


def _close(got, want, rel=1e-6):
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    assert np.all(np.abs(got - want) <= rel * np.abs(want) + 1e-12 * max(1.0, float(np.abs(want).max()))), \
        float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-30)))


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("geom,model", [("trench3d", "diffuse"), ("trench2d", "diffuse"), ("mesh", "diffuse"),
                                        ("trench3d", "coned"), ("trench2d", "coned")])
def test_inert_state_is_invisible(geom, model, model_cache, monkeypatch):
    """A stateful wrapper of ModelDiffuse / ModelConedCosine (state carried, never read; init draws nothing) traces the
    built-in particle's rays: flux and every counter bit-equal to the built-in device particle, and the oracle's."""
    monkeypatch.setenv("VR_CACHE_DIR", model_cache)
    t, o, _ = _scene(geom)
    _rays(t, o, 150_000, 913)
    base = "ModelDiffuse" if model == "diffuse" else "ModelConedCosine"
    k = t.registerParticleModel(INERT % {"base": base}, numData=1, name="inert", numState=1)
    if model == "diffuse":
        builtin = vr.DiffuseParticle(0.3, "flux")
        user = vr.UserModelParticle(k, 0.3, ["flux"])
        o.set_particle(po.DIFFUSE, 0.3)
    else:
        builtin = vr.ConedCosineParticle(0.3, 1.0, 0.6, "flux")
        user = vr.UserModelParticle(k, 0.3, ["flux"], params=[0.6])
        o.set_particle_ex(po.CONED_COSINE, 0.3, 1.0, 0.6)

    def run(particle):
        t.setParticleType(particle)
        t.setRunNumber(1)
        t.apply()
        return t.traceMode(), info_dict(t), t.getLocalData().getVectorData(0).copy()
    m_user, i_user, f_user = run(user)
    m_ref, i_ref, f_ref = run(builtin)
    assert m_user == {"trench2d": 4}.get(geom, 0)          # MODE 4 (LDS-resident scene) on the 2-D trench, else MODE 0
    assert i_user == i_ref and (f_user == f_ref).all()
    o.apply(po.max_threads())
    oi = o.info()
    assert all(i_user[key] == oi[key] for key in INFO_KEYS), (i_user, oi)
    assert l2_rel(f_user, o.flux()) <= 5e-6


@pytest.mark.gpu
def test_state_follows_the_ray_and_resets(model_cache, monkeypatch):
    """A hit counter in the state, on a triangle trench (no neighbour credits: every credit is one logged surface hit).
    Label 0 (w) against the oracle; labels 1 (w of first hits) and 2 (w x hit number) against the sums rebuilt from the
    oracle's event log.  A million rays: every lane of the persistent kernel picks up several rays in turn."""
    monkeypatch.setenv("VR_CACHE_DIR", model_cache)
    t, o, tri = _mesh()
    nr = 1_000_000
    _rays(t, o, nr, 4242)
    k = t.registerParticleModel(HIT_COUNTER, numData=3, name="hits", numState=1)
    t.setParticleType(vr.UserModelParticle(k, 0.3, ["w", "first", "nth"]))
    t.apply()
    ld = t.getLocalData()
    f = [ld.getVectorData(i).copy() for i in range(3)]
    gi = info_dict(t)
    o.set_particle(po.DIFFUSE, 0.3)
    o.set_event_capacity(200_000_000)
    o.apply(1)
    oi = o.info()
    assert all(gi[key] == oi[key] for key in INFO_KEYS), (gi, oi)
    assert l2_rel(f[0], o.flux()) <= 5e-6
    ray, prim, w, nth = _surface_events(o)
    assert ray.size == gi["geometryHits"] and nth.max() > 5
    n = len(tri)
    w64 = w.astype(np.float64)
    _close(f[0], np.bincount(prim, weights=w64, minlength=n))
    _close(f[1], np.bincount(prim, weights=np.where(nth == 1, w64, 0.0), minlength=n))
    _close(f[2], np.bincount(prim, weights=(w * nth.astype(np.float32)).astype(np.float64), minlength=n))
    assert not (f[2] == f[0]).all()                         # (the counter really counts)


@pytest.mark.gpu
@pytest.mark.parametrize("draws,primary", [(0, False), (1, False), (3, False), (1, True)])
def test_init_comes_before_the_source_and_consumes_the_engine(draws, primary, model_cache, monkeypatch):
    """init draws K engine outputs BEFORE the source sample: the generator's first rays (vr_debug_model_source_sample:
    origin, direction and the draws consumed) fed to the oracle as host rays with those draw counts give the device
    apply's flux and counters.  K = 0: the rays of the library's own generator, bit for bit."""
    monkeypatch.setenv("VR_CACHE_DIR", model_cache)
    t, o, _ = _disks("trench3d")
    nr, seed = 120_000, 77
    _rays(t, o, nr, seed)
    if primary:
        t.setPrimaryDirection([0.2, 0.1, -1.0])
    k = t.registerParticleModel(INIT_DRAWS, numData=1, name="initDraws", numState=2)
    t.setParticleType(vr.UserModelParticle(k, 0.4, ["flux"], params=[float(draws)]))
    idx = np.arange(nr, dtype=np.uint64)
    org, d, used = t.debugModelSourceSample(idx, seed + 1)   # (the apply's kernel seed: rngSeed + runNumber)
    assert used.min() >= draws + 4
    if not primary:
        assert (used == draws + 4).all()
    if draws == 0 and not primary:
        o0, d0 = t.debugSourceSample(idx, seed + 1)
        assert (o0 == org).all() and (d0 == d).all()
    else:
        assert not (d == t.debugSourceSample(idx, seed + 1)[1]).all()
    t.apply()
    f = t.getLocalData().getVectorData(0).copy()
    gi = info_dict(t)
    o.set_particle(po.DIFFUSE, 0.4)
    o.set_host_rays(org, d)
    o.set_host_ray_draws(used)
    o.apply(po.max_threads())
    oi = o.info()
    assert all(gi[key] == oi[key] for key in INFO_KEYS), (gi, oi)
    assert l2_rel(f, o.flux()) <= 5e-6


@pytest.mark.gpu
def test_material_id_reaches_the_hooks(model_cache, monkeypatch):
    """collide sees the material id of the credited primitive (label 1 = label 0 masked by the material map, bit for
    bit) and surface_reflection that of the hit one (sticking only on material 2 = the oracle with the material
    sticking map {2: 1.0}, others 0)."""
    monkeypatch.setenv("VR_CACHE_DIR", model_cache)
    t, o, p = _disks("trench3d")
    _rays(t, o, 150_000, 99)
    mats = (np.arange(len(p)) % 3).astype(np.int32)
    t.setMaterialIds(mats)
    o.set_material_ids(mats)
    k = t.registerParticleModel(MATERIAL, numData=2, name="material", numState=1)
    t.setParticleType(vr.UserModelParticle(k, 0.3, ["all", "mat1"], params=[0.0]))
    t.apply()
    ld = t.getLocalData()
    f0, f1 = ld.getVectorData(0).copy(), ld.getVectorData(1).copy()
    assert (f1 == np.where(mats == 1, f0, 0.0)).all() and f1.sum() > 0
    t.setParticleType(vr.UserModelParticle(k, 0.0, ["all", "mat1"], params=[1.0]))
    t.setRunNumber(1)
    t.apply()
    f = t.getLocalData().getVectorData(0).copy()
    gi = info_dict(t)
    o.set_particle(po.DIFFUSE, 0.0)
    o.set_material_sticking({2: 1.0})
    o.apply(po.max_threads())
    oi = o.info()
    assert all(gi[key] == oi[key] for key in INFO_KEYS), (gi, oi)
    assert l2_rel(f, o.flux()) <= 5e-6


@pytest.mark.gpu
def test_energy_known_answer(model_cache, monkeypatch):
    """init sets E = E0 without draws, every hit halves E and the particle sticks once E < Emin, reflecting specularly
    before: every ray ends at its m-th surface hit, m = ceil(log2(E0 / Emin)), or leaves earlier.  Against the oracle's
    specular particle (sticking 0) whose event log is cut after each ray's m-th surface hit: counters, the flux and the
    energies credited."""
    monkeypatch.setenv("VR_CACHE_DIR", model_cache)
    t, o, tri = _mesh()
    nr, e0, emin = 300_000, 1.0, 0.2
    m = int(np.ceil(np.log2(e0 / emin)))
    _rays(t, o, nr, 555)
    k = t.registerParticleModel(ENERGY, numData=2, name="energy", numState=1)
    t.setParticleType(vr.UserModelParticle(k, 0.0, ["hits", "energy"], params=[e0, emin]))
    t.apply()
    ld = t.getLocalData()
    f0, f1 = ld.getVectorData(0).copy(), ld.getVectorData(1).copy()
    gi = info_dict(t)
    o.set_particle(po.SPECULAR, 0.0)
    o.set_event_capacity(100_000_000)
    o.apply(1)
    ev = o.events()
    ray, kind = ev["ray"], ev["kind"]
    surf = (kind == 3).astype(np.int64)
    start = np.r_[True, ray[1:] != ray[:-1]]
    seg = np.cumsum(start) - 1
    cum = np.cumsum(surf)
    before = cum - surf - np.r_[0, cum][np.flatnonzero(start)][seg]   # surface hits of the ray before this event
    keep = before < m                                             # the events up to and including the m-th surface hit
    hits = np.bincount(seg[keep], weights=surf[keep], minlength=seg.max() + 1).astype(np.int64)
    assert hits.max() == m and gi["numRays"] == nr
    assert gi["geometryHits"] == int(hits.sum())
    assert gi["reflections"] == int(np.minimum(hits, m - 1).sum())
    assert gi["nonGeometryHits"] == int(((kind == 0) & keep).sum())
    assert gi["boundaryHits"] == int(((kind == 1) & keep).sum())
    sel = keep & (kind == 3)
    prim = ev["prim"][sel].astype(np.int64)
    nth = before[sel] + 1
    n = len(tri)
    _close(f0, np.bincount(prim, weights=ev["weight"][sel].astype(np.float64), minlength=n))
    _close(f1, np.bincount(prim, weights=e0 * 0.5 ** (nth - 1), minlength=n))


@pytest.mark.gpu
def test_stateful_refusals(model_cache, monkeypatch):
    """numState outside 0 .. 4, numState != kStateWords, and sources other than SourceRandom are refused clearly."""
    monkeypatch.setenv("VR_CACHE_DIR", model_cache)
    t, o, p = _disks("trench3d")
    _rays(t, o, 10_000, 1)
    with pytest.raises(vr.VrError, match="0 .. 4"):
        t.registerParticleModel(INIT_DRAWS, numData=1, numState=5)
    with pytest.raises(vr.VrError, match="kStateWords differs"):
        t.registerParticleModel(INIT_DRAWS, numData=1, numState=1)
    k = t.registerParticleModel(INIT_DRAWS, numData=1, name="initDraws", numState=2)
    t.setParticleType(vr.UserModelParticle(k, 0.4, ["flux"], params=[1.0]))
    t.setSource(vr.SourceGrid(p[:64] + np.array([0.0, 0.0, 5.0], dtype=np.float32)))
    with pytest.raises(vr.VrError, match="SourceRandom only"):
        t.apply()
    t2, _, p2 = _disks("trench3d")
    t2.setNumberOfRaysFixed(1000)
    t2.setParticleType(vr.UserModelParticle(t2.registerParticleModel(INIT_DRAWS, numData=1, numState=2), 0.4, ["f"]))
    org, d = np.tile([[0.0, 0.0, 5.0]], (1000, 1)), np.tile([[0.0, 0.0, -1.0]], (1000, 1))
    t2.setHostRays(org, d)
    with pytest.raises(vr.VrError, match="SourceRandom only"):
        t2.apply()


# ---------------------------------------------------------------------------------------------------------------------
def _compile_module(tmp_path, model, num_state):
    """the translation unit vr_register_particle_model writes, compiled for gfx950 (no device needed)"""
    (tmp_path / "model.hpp").write_text(model)
    tu = tmp_path / "module.hip"
    tu.write_text(f"#define VR_USER_MODULE 1\n#define VR_USER_NUM_DATA 1\n#define VR_USER_NUM_STATE {num_state}\n"
                  f"#define VR_USER_MODEL_FILE \"{tmp_path / 'model.hpp'}\"\n#include <cstddef>\n"
                  f"#include \"{CSRC}/vr_trace.hip\"\n")
    hipcc = os.environ.get("VR_HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "--genco", "--offload-arch=gfx950", "-O0", "-std=c++17", "-fsyntax-only", "-I", CSRC,
                        str(tu), "-o", str(tmp_path / "module.hsaco")], capture_output=True, text=True)
    return r.returncode, r.stdout + r.stderr


def test_stateful_model_shape_is_checked_at_compile_time(tmp_path):
    """numState must be kStateWords, kStateWords at most 4, and a stateful model must be a kNeedsFull one: the module's
    static_asserts say so (checked without a device)."""
    rc, out = _compile_module(tmp_path, INIT_DRAWS, 1)
    assert rc != 0 and "kStateWords differs from the numState given at registration" in out
    rc, out = _compile_module(tmp_path, INIT_DRAWS.replace("kStateWords = 2", "kStateWords = 5"), 5)
    assert rc != 0 and "0 .. 4 state words" in out
    rc, out = _compile_module(tmp_path, INIT_DRAWS.replace("kNeedsFull = true", "kNeedsFull = false"), 2)
    assert rc != 0 and "needs kNeedsFull = true" in out
    rc, out = _compile_module(tmp_path, INIT_DRAWS, 2)
    assert rc == 0, out
