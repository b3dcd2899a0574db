"""Flux statistics (Trace.setCalculateFluxError, vr_set_flux_statistics): per-primitive hit counts, the sum of the squared
credits and the Monte-Carlo error made from them.

The sums are integers (hits in units of one, the squares at 2^-40 like the flux), so everything that can be exact is
compared exactly: hit counts against the oracle's event log and against a run-time model that counts for itself, the
shards of a sharded apply against the whole, the absorbing launches' planes against their flux.  Sums of squares
rebuilt elsewhere (float64 squares of the event log's weights, a user model's float32 squares) are compared to 1e-6
relative, the rule of test_stateful_models.py for sums rebuilt from events.  Flux and counters with statistics on are
bit-equal to the same apply with statistics off throughout."""
import numpy as np
import pytest

import viennaray_amd as vr
from viennaray_amd import BoundaryCondition as BC, TraceDirection as TD
from oracle import pyoracle as po
from helpers import trench2d, trench3d, trench_mesh

pytestmark = pytest.mark.gpu

INFO_KEYS = ("numRays", "totalRaysTraced", "nonGeometryHits", "geometryHits", "particleHits",
             "boundaryHits", "reflections", "raysTerminated")


def info_dict(t, q=None):
    i = t.getRayTraceInfo() if q is None else t.getParticleTraceInfo(q)
    return {k: int(getattr(i, k)) for k in INFO_KEYS}


def _surface_events(o):
    """kind-3 events (surface hits) of the oracle's log: ray, primitive, weight (tests/test_stateful_models.py)"""
    ev = o.events()
    sel = ev["kind"] == 3
    ray, prim, w = ev["ray"][sel], ev["prim"][sel].astype(np.int64), ev["weight"][sel]
    order = np.argsort(ray, kind="stable")
    return ray[order], prim[order], w[order]


def _close(got, want, rel=1e-6):
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    assert np.all(np.abs(got - want) <= rel * np.abs(want) + 1e-12 * max(1.0, float(np.abs(want).max()))), \
        float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-30)))


@pytest.fixture(scope="module")
def model_cache(tmp_path_factory):
    """one code-object cache for the module: each model is compiled once"""
    return str(tmp_path_factory.mktemp("vr_stats_cache"))


def _plane(n=64, ripple=0.0):
    """n x n plane of disks, optionally rippled by `ripple` grid cells (tools/case_bench.py's sheet)"""
    ax = np.arange(n) - (n - 1) / 2.0
    x, y = np.meshgrid(ax, ax, indexing="ij")
    wave = 4.0
    z = ripple * np.sin(x / wave) * np.cos(y / wave)
    nrm = np.stack([-ripple / wave * np.cos(x / wave) * np.cos(y / wave), ripple / wave * np.sin(x / wave) * np.sin(y / wave),
                    np.ones_like(x)], -1).reshape(-1, 3)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32), nrm.astype(np.float32)


def _disk_tracer(geom):
    if geom == "trench3d":
        gd, p, n = trench3d()
        t = vr.TraceDisk(3)
        t.setGeometry(p, n, gd)
        t.setBoundaryConditions([BC.PERIODIC_BOUNDARY] * 3)
    elif geom == "trench2d":
        gd, p, n = trench2d()
        t = vr.TraceDisk(2)
        t.setGeometry(p, n, gd)
        t.setSourceDirection(TD.POS_Y)
        t.setBoundaryConditions([BC.PERIODIC_BOUNDARY] * 2)
    else:
        p, n = _plane(64, 0.5 if geom == "ripple" else 0.0)
        t = vr.TraceDisk(3)
        t.setGeometry(p, n, 1.0)
        t.setBoundaryConditions([BC.REFLECTIVE_BOUNDARY] * 3)
    return t, len(p)


def _mesh_tracer():
    gd, v, tri = trench_mesh()
    t = vr.TraceTriangle(3)
    t.setGeometry(v, tri, gd)
    return t, (gd, v, tri)


def _apply(t, seed, run=1):
    t.setRngSeed(seed)
    t.setRunNumber(run)
    t.apply()


def _labels(t):
    ld = t.getLocalData()
    return [ld.getVectorData(i).copy() for i in range(t.numData())]


# ---------------------------------------------------------------------------------------------------------------------
# 1. triangles against the oracle's event log
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["diffuse", "specular"])
def test_triangles_against_the_event_log(kind):
    t, (gd, v, tri) = _mesh_tracer()
    particle = vr.DiffuseParticle(0.3, "flux") if kind == "diffuse" else vr.SpecularParticle(0.3, 1.0, "flux")
    t.setParticleType(particle)
    t.setNumberOfRaysFixed(200_000)
    _apply(t, 77)
    off = (t.traceMode(), info_dict(t), _labels(t)[0], t.getFluxF64())
    t.setCalculateFluxError(True)
    _apply(t, 77)
    on = (t.traceMode(), info_dict(t), _labels(t)[0], t.getFluxF64())
    assert on[1] == off[1] and (on[2] == off[2]).all() and (on[3] == off[3]).all()
    hits, sumsq = t.getHitCounts(), t.getFluxSumSquares()

    o = po.Oracle()
    o.set_triangles(v, tri, gd, 3)
    o.set_particle(po.DIFFUSE if kind == "diffuse" else po.SPECULAR, 0.3, 1.0)
    o.set_num_rays_fixed(200_000)
    o.set_rng_seed(77)
    o.set_lazy_rng(True)
    o.set_event_capacity(50_000_000)
    o.apply(1)
    oi = o.info()
    assert all(on[1][k] == oi[k] for k in INFO_KEYS), (on[1], oi)
    _, prim, w = _surface_events(o)
    n = len(tri)
    assert prim.size == on[1]["geometryHits"]
    assert (hits == np.bincount(prim, minlength=n).astype(np.uint64)).all()
    _close(sumsq, np.bincount(prim, weights=w.astype(np.float64) ** 2, minlength=n))
    assert hits.dtype == np.uint64 and int(hits.sum()) == prim.size and hits.max() > 1


# ---------------------------------------------------------------------------------------------------------------------
# 2. absorbing disks: the kernels of today, hits = sumsq = flux
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ["trench3d", "trench2d", "plane"])
def test_absorbing_launches_keep_their_kernels(geom):
    t, n = _disk_tracer(geom)
    t.setParticleType(vr.DiffuseParticle(1.0, "flux"))
    t.setNumberOfRaysFixed(100_000)
    _apply(t, 5)
    off = (t.traceMode(), info_dict(t), t.getFluxF64())
    t.setCalculateFluxError(True)
    _apply(t, 5)
    on = (t.traceMode(), info_dict(t), t.getFluxF64())
    assert on[0] == off[0] and (on[0] == 4 if geom == "trench2d" else on[0] in (1, 2, 5))   # (an absorbing kernel; MODE_SMALL in 2-D)
    assert on[1] == off[1] and (on[2] == off[2]).all()
    hits, sumsq = t.getHitCounts(), t.getFluxSumSquares()
    assert (hits.astype(np.float64) == sumsq).all() and (sumsq == on[2]).all() and hits.sum() >= on[1]["geometryHits"]
    # unit weights: sigma^2 = S1 - S1^2 / N
    s1 = on[2]
    want = np.sqrt(np.maximum(s1 - s1 * s1 / 100_000.0, 0.0))
    assert np.allclose(t.getFluxAbsoluteError(), want, rtol=1e-6, atol=0)


def test_weighted_host_rays_take_the_general_path():
    """start weights 0.5 / 2.0 on the flat plane: the launch is no longer absorbing, sumsq = w^2 hits and S1 = w hits,
    exact in fixed point"""
    t, n = _disk_tracer("plane")
    t.setParticleType(vr.DiffuseParticle(1.0, "flux"))
    t.setCalculateFluxError(True)
    rng = np.random.default_rng(3)
    m = 20_000
    org = np.stack([rng.uniform(-30, 30, m), rng.uniform(-30, 30, m), np.full(m, 0.5)], 1).astype(np.float32)
    d = np.stack([rng.uniform(-0.3, 0.3, m), rng.uniform(-0.3, 0.3, m), np.full(m, -1.0)], 1)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    res = {}
    for w in (0.5, 2.0):
        t.setHostRays(org, d, weights=np.full(m, w, dtype=np.float32))
        _apply(t, 9)
        assert t.traceMode() not in (1, 2, 5)
        hits = t.getHitCounts().astype(np.float64)
        assert hits.sum() >= m and (t.getFluxSumSquares() == w * w * hits).all() and (t.getFluxF64() == w * hits).all()
        res[w] = hits
    assert (res[0.5] == res[2.0]).all()


# ---------------------------------------------------------------------------------------------------------------------
# 3. every credit path against a user model that keeps the sums itself
# ---------------------------------------------------------------------------------------------------------------------
SELF_COUNTING = """
struct VrUserModel : %(base)s {
  static constexpr int kNumData = 3;
  static constexpr bool kNeedsFull = %(full)s;
  template <class Credit>
  __device__ static void collide(const ModelCtx &m, float w, const V3 &d, const V3 &n, unsigned primID, Credit &&credit) {
    %(base)s::collide(m, w, d, n, primID, [&](int label, float v) {
      if (label == 0) {
        credit(0, v);
        credit(1, v * v);
        credit(2, 1.f);
      }
    });
  }
};
"""

CASES = {
    # name: (geometry, built-in particle, model base, particle params of the user model, needsFull, wdist)
    "trench3d": ("trench3d", lambda: vr.DiffuseParticle(0.1, "flux"), "ModelDiffuse", (), False, False),
    "wdist": ("trench3d", lambda: vr.DiffuseParticle(0.1, "flux"), "ModelDiffuse", (), True, True),
    "coned": ("trench3d", lambda: vr.ConedCosineParticle(0.1, 1.0, 0.6, "flux"), "ModelConedCosine", (0.6,), True, False),
    "small2d": ("trench2d", lambda: vr.DiffuseParticle(0.1, "flux"), "ModelDiffuse", (), False, False),
    "plane": ("plane", lambda: vr.DiffuseParticle(0.1, "flux"), "ModelDiffuse", (), False, False),
    "ripple": ("ripple", lambda: vr.DiffuseParticle(0.1, "flux"), "ModelDiffuse", (), False, False),
    "cosine2": ("trench3d", lambda: vr.DiffuseCosineParticle(0.1, "flux", "cos"), "ModelDiffuseCosine", (), False, False),
}


def _register(t, base, full):
    return t.registerParticleModel(SELF_COUNTING % {"base": base, "full": "true" if full else "false"}, numData=3,
                                   needsFull=full, name="selfcount")


@pytest.mark.parametrize("case", list(CASES))
def test_credit_paths_against_a_self_counting_model(case, model_cache, monkeypatch):
    monkeypatch.setenv("VR_CACHE_DIR", model_cache)
    geom, builtin, base, params, full, wdist = CASES[case]
    t, n = _disk_tracer(geom)
    t.setUseWdist(wdist)
    t.setNumberOfRaysFixed(150_000)
    k = _register(t, base, full)
    sp = builtin().getSourceDistributionPower()
    t.setParticleType(vr.UserModelParticle(k, 0.1, ["w", "w2", "n"], sourcePower=sp, params=params))
    _apply(t, 31)
    user = (info_dict(t), t.getFluxF64(), _labels(t))
    t.setParticleType(builtin())
    _apply(t, 31)
    off = (t.traceMode(), info_dict(t), _labels(t))
    t.setCalculateFluxError(True)
    _apply(t, 31)
    on = (t.traceMode(), info_dict(t), _labels(t), t.getFluxF64())
    if case == "small2d":
        assert on[0] == off[0] == 4
    if case == "plane":
        assert on[0] == 3      # the packet query's crediting
    assert on[1] == off[1] == user[0]
    assert len(on[2]) == len(off[2]) and all((a == b).all() for a, b in zip(on[2], off[2]))
    assert (on[3] == user[1]).all()
    hits, sumsq = t.getHitCounts(), t.getFluxSumSquares()
    assert (hits.astype(np.float64) == user[2][2].astype(np.float64)).all() and hits.sum() > on[1]["geometryHits"] // 2
    _close(sumsq, user[2][1].astype(np.float64), rel=1e-6)   # (float square against double square)
    assert hits.max() < 2 ** 24    # (the user model's float label holds its count exactly)


def test_particle_list_keeps_statistics_per_particle(model_cache, monkeypatch):
    monkeypatch.setenv("VR_CACHE_DIR", model_cache)
    t, n = _disk_tracer("trench3d")
    t.setNumberOfRaysFixed(150_000)
    kd = _register(t, "ModelDiffuse", False)
    ks = _register(t, "ModelSpecular", False)
    t.setParticleTypes([vr.UserModelParticle(kd, 0.1, ["w", "w2", "n"]),
                        vr.UserModelParticle(ks, 0.3, ["sw", "sw2", "sn"], sourcePower=1.0)])
    _apply(t, 47)
    user = (_labels(t), [info_dict(t, q) for q in range(2)])
    t.setParticleTypes([vr.DiffuseParticle(0.1, "a"), vr.SpecularParticle(0.3, 1.0, "b")])
    t.setCalculateFluxError(True)
    _apply(t, 47)
    flux = _labels(t)
    assert len(flux) == 2 and [info_dict(t, q) for q in range(2)] == user[1]
    for q in range(2):
        assert (flux[q] == user[0][3 * q]).all()
        assert (t.getHitCounts(q).astype(np.float64) == user[0][3 * q + 2].astype(np.float64)).all()
        _close(t.getFluxSumSquares(q), user[0][3 * q + 1].astype(np.float64), rel=1e-6)
    assert not (t.getHitCounts(0) == t.getHitCounts(1)).all()
    ptr, words = t.fluxAccumulators()
    assert words == n * 6 and t.numAccumulatorPlanes() == 6


def test_run_time_model_with_statistics(model_cache, monkeypatch):
    """a run-time model itself under statistics: its twin module, compiled on first use, counts what the model counts"""
    monkeypatch.setenv("VR_CACHE_DIR", model_cache)
    t, n = _disk_tracer("trench2d")
    t.setNumberOfRaysFixed(50_000)
    src = """
struct VrUserModel : ModelDiffuse {
  static constexpr int kNumData = 2;
  template <class Credit>
  __device__ static void collide(const ModelCtx &, float w, const V3 &, const V3 &, unsigned, Credit &&credit) {
    credit(0, 0.5f * w);
    credit(1, 1.f);
  }
};
"""
    k = t.registerParticleModel(src, numData=2, name="half")
    t.setParticleType(vr.UserModelParticle(k, 0.2, ["half", "n"]))
    _apply(t, 8)
    off = (info_dict(t), _labels(t))
    t.setCalculateFluxError(True)
    _apply(t, 8)
    assert info_dict(t) == off[0] and all((a == b).all() for a, b in zip(_labels(t), off[1]))
    assert (t.getHitCounts().astype(np.float64) == off[1][1].astype(np.float64)).all()
    assert t.getHitCounts().sum() > 0


# ---------------------------------------------------------------------------------------------------------------------
# 4. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals(model_cache, monkeypatch):
    monkeypatch.setenv("VR_CACHE_DIR", model_cache)
    t, n = _disk_tracer("trench2d")
    t.setNumberOfRaysFixed(10_000)
    t.setParticleType(vr.DiffuseParticle(0.5, "flux"))
    with pytest.raises(vr.VrError, match="statistics are off"):
        t.getHitCounts()
    _apply(t, 1)
    for getter in (t.getHitCounts, t.getFluxSumSquares, t.getFluxRelativeError, t.getFluxAbsoluteError, t.getFluxErrorTensor):
        with pytest.raises(vr.VrError, match="statistics are off"):
            getter()
    t.setCalculateFluxError(True)
    with pytest.raises(vr.VrError, match="no result"):   # (before any apply with statistics)
        t.getHitCounts()
    t.applyPrepare()
    t.applyLaunch()
    with pytest.raises(vr.VrError, match="no result"):   # (launched, not finished)
        t.getFluxRelativeError()
    t.applyFinish(collect=False)
    assert t.getHitCounts().shape == (n,)
    with pytest.raises(vr.VrError, match="particleIdx"):
        t.getHitCounts(1)
    import ctypes as C
    out = np.empty(n + 1, dtype=np.uint64)
    assert t._L.vr_get_hit_counts(t._h, 0, C.c_void_p(out.ctypes.data), n + 1) != 0
    assert b"size mismatch" in t._L.vr_last_error(t._h)
    out4 = np.empty(n, dtype=np.float32)
    assert t._L.vr_get_flux_error(t._h, 0, 0, C.c_void_p(out4.ctypes.data), n - 1) != 0
    assert b"size mismatch" in t._L.vr_last_error(t._h)
    # a model with three data labels has no room for the two companion planes
    k = _register(t, "ModelDiffuse", False)
    t.setParticleType(vr.UserModelParticle(k, 0.5, ["w", "w2", "n"]))
    with pytest.raises(vr.VrError, match=r"at most 2 data labels"):
        t.applyPrepare()
    t.setCalculateFluxError(False)
    t.applyPrepare()                                      # (the same model without statistics is fine)


# ---------------------------------------------------------------------------------------------------------------------
# 5. integers add up across shards
# ---------------------------------------------------------------------------------------------------------------------
def test_shards_add_up_bit_for_bit():
    import torch
    t, (gd, v, tri) = _mesh_tracer()
    n = len(tri)
    t.setParticleType(vr.DiffuseParticle(0.3, "flux"))
    t.setNumberOfRaysFixed(200_000)
    t.setCalculateFluxError(True)
    _apply(t, 77)
    ptr, words = t.fluxAccumulators()
    assert words == 3 * n
    whole = (t.getFluxF64(), t.getHitCounts(), t.getFluxSumSquares(), t.getFluxRelativeError(), t.getFluxAbsoluteError())
    acc = torch.zeros(3 * n, dtype=torch.int64, device="cuda")
    t.bindFluxAccumulators(acc.data_ptr(), 3 * n)
    t.setWorldSize(2)
    total = torch.zeros_like(acc)
    for first in (0, 100_000):
        t.setRayRange(first, 100_000)
        _apply(t, 77)
        torch.cuda.synchronize()
        total += acc
    acc.copy_(total)                      # what an all-reduce leaves in the bound buffer
    torch.cuda.synchronize()
    t.setRayRange(0, 0)
    assert (t.getFluxF64() == whole[0]).all() and (t.getHitCounts() == whole[1]).all() and (t.getFluxSumSquares() == whole[2]).all()
    # N is the whole apply's ray count, not a shard's: the summed shards give the single apply's error, bit for bit
    assert np.array_equal(t.getFluxRelativeError().view(np.uint32), whole[3].view(np.uint32))
    assert np.array_equal(t.getFluxAbsoluteError().view(np.uint32), whole[4].view(np.uint32))
    from viennaray_amd.distributed import flux_statistics_from_accumulators
    hits, rel = flux_statistics_from_accumulators(total, n, [1], 200_000)
    assert (hits[0] == whole[1]).all() and np.allclose(rel[0], whole[3], rtol=1e-6)


# ---------------------------------------------------------------------------------------------------------------------
# 6. device getter
# ---------------------------------------------------------------------------------------------------------------------
def test_device_getter_and_unreached_primitives():
    import torch
    p, nrm = _plane(16)
    hidden = len(p)                      # a disk under the closed plane: no ray reaches it
    p = np.vstack([p, [[0.25, 0.25, -2.0]]]).astype(np.float32)
    nrm = np.vstack([nrm, [[0.0, 0.0, 1.0]]]).astype(np.float32)
    t = vr.TraceDisk(3)
    t.setGeometry(torch.from_numpy(p).cuda(), torch.from_numpy(nrm).cuda(), 1.0)
    t.setBoundaryConditions([BC.REFLECTIVE_BOUNDARY] * 3)
    t.setParticleType(vr.DiffuseParticle(0.4, "flux"))
    t.setNumberOfRaysFixed(60_000)
    t.setCalculateFluxError(True)
    t.setRngSeed(13)
    t.apply(collect=False)
    rel_d, abs_d = t.getFluxErrorTensor(0, "relative"), t.getFluxErrorTensor(0, "absolute")
    assert rel_d.dtype == torch.float32 and rel_d.is_cuda and rel_d.shape == (len(p),)
    rel_h, abs_h = t.getFluxRelativeError(), t.getFluxAbsoluteError()
    assert np.array_equal(rel_d.cpu().numpy().view(np.uint32), rel_h.view(np.uint32))
    assert np.array_equal(abs_d.cpu().numpy().view(np.uint32), abs_h.view(np.uint32))
    hits = t.getHitCounts()
    assert hits[hidden] == 0 and hits[:hidden].min() > 0
    assert np.isposinf(rel_h[hidden]) and abs_h[hidden] == 0 and np.isfinite(rel_h[:hidden]).all()
    # the definition, in double
    s1, sq = t.getFluxF64(), t.getFluxSumSquares()
    sigma = np.sqrt(np.maximum(sq - s1 * s1 / 60_000.0, 0.0))
    assert np.allclose(abs_h, sigma, rtol=1e-6, atol=0)
    assert np.allclose(rel_h[:hidden], sigma[:hidden] / s1[:hidden], rtol=1e-6, atol=0)
    with pytest.raises(ValueError):
        t.getFluxErrorTensor(0, "variance")


# ---------------------------------------------------------------------------------------------------------------------
# 7. the estimate means what it says
# ---------------------------------------------------------------------------------------------------------------------
def test_predicted_error_matches_the_scatter_of_the_runs():
    """24 runs of the scene of test 1: the pooled ratio of the empirical standard deviation of the raw flux over the
    runs to the predicted sigma is within 3 % of 1 (the oracle's own value for this input: 0.996, see
    test_flux_statistics_host.py; sampling error of the pooled ratio about 0.2 %)."""
    import math
    t, (gd, v, tri) = _mesh_tracer()
    t.setParticleType(vr.DiffuseParticle(0.3, "flux"))
    t.setNumberOfRaysFixed(200_000)
    t.setCalculateFluxError(True)
    t.setRngSeed(77)
    flux, var = [], []
    for run in range(24):
        t.setRunNumber(run)
        t.apply(collect=False)
        flux.append(t.getFluxF64())
        var.append(t.getFluxAbsoluteError().astype(np.float64) ** 2)
    flux, var = np.array(flux), np.array(var)
    pool = flux.mean(axis=0) != 0
    assert pool.mean() >= 0.99
    emp = flux.std(axis=0, ddof=1)[pool]
    pred = np.sqrt(var.mean(axis=0))[pool]
    ratio = float(np.sqrt((emp ** 2).sum() / (pred ** 2).sum()))
    print(f"pooled emp / pred = {ratio:.4f} over {int(pool.sum())} of {pool.size} triangles")
    assert 0.97 <= ratio <= 1.03, ratio
    # the ray count an adaptive loop would ask for
    rel = t.getFluxRelativeError()
    q = float(np.quantile(rel[np.isfinite(rel)].astype(np.float64), 0.95))
    assert t.raysForRelativeError(0.05) == math.ceil(200_000 * (q / 0.05) ** 2)
    q50 = float(np.quantile(rel[np.isfinite(rel)].astype(np.float64), 0.5))
    assert t.raysForRelativeError(0.1, quantile=0.5) == math.ceil(200_000 * (q50 / 0.1) ** 2)
