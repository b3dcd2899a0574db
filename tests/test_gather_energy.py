"""gatherEnergy on the device (vr_gather_energy*, vr_debug_gather_energy_path; Trace.gatherEnergy, gatherEnergyAdaptive,
gatherEnergySums, debugGatherEnergyPath): gatherAngular with an ion's energy carried along every path — E0 drawn at the
source, a share eps(mu) kept at every reflection, one more multiply by the yield at the arrival energy.  The three
identities with gatherAngular for every form, cut on = cut off bit for bit (with paths the cut really ended), single paths
replayed in numpy float32 multiply by multiply, range splits, entry points, the adaptive call, a closed form that goes
through no other gather, the refusals, an apply left as it was and the C++ façade.  The scenes are the neighbours' smallest:
the trench mesh and the 2-D disk trench."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import viennaray_amd as vr
from viennaray_amd import capi
import closed_forms as cf
from test_gather_energy_host import energy_u, law

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BC = vr.BoundaryCondition
GR = vr.GatherReflection
SEED = 7
ONE = np.float32(1.0)
KINDS = [GR.SPECULAR, GR.DIFFUSE]
R5 = np.linspace(1.0, 0.2, 5).astype(np.float32)    # a reflectivity law
Y5 = np.linspace(0.5, 3.0, 5).astype(np.float32)    # an angular yield
EPS = np.linspace(1.0, 0.3, 8).astype(np.float32)   # the retention law: falling to 0.3 at normal incidence
YE = np.array([0.0, 0.0, 1.0], np.float32)          # the yield by energy: a threshold at half of energyMax
Q3 = np.array([30.0, 60.0, 100.0], np.float32)      # the source's quantiles, energyMax = 100
ION = dict(energyYield=YE, energyMax=100.0, sourceQuantiles=Q3, retentionLaw=EPS)
I64 = C.POINTER(C.c_int64)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _prepared(t):
    t.setParticleType(vr.DiffuseParticle(1.0, "flux"))
    t.setNumberOfRaysFixed(1000)
    t.setRngSeed(SEED)
    t.applyPrepare()
    return t


def _mesh_tracer(g):
    t = vr.TraceTriangle(3)
    t.setGeometry(g.verts, g.tris, 1.0)
    t.setBoundaryConditions([BC.REFLECTIVE_BOUNDARY, BC.PERIODIC_BOUNDARY, BC.REFLECTIVE_BOUNDARY])
    return t


@functools.lru_cache(maxsize=None)
def _mesh():
    """the trench mesh with a wall budget no path of the tests below can spend; coord: x on the bottom, z on the walls"""
    g = cf.trench_mesh()
    cen, _ = cf.triangle_centroids(g)
    coord = np.where(g.part == cf.BOTTOM, cen[:, 0], cen[:, 2])
    t = _mesh_tracer(g)
    t.setMaxBoundaryHits(1 << 16)
    return _prepared(t), g, coord


@functools.lru_cache(maxsize=None)
def _disks2():
    g = cf.trench_disks(2)
    t = vr.TraceDisk(2)
    t.setGeometry(g.points, g.normals, 1.0)
    t.setBoundaryConditions([BC.REFLECTIVE_BOUNDARY, BC.REFLECTIVE_BOUNDARY])
    t.setSourceDirection(cf.POS_Y)
    return _prepared(t), g


def _scene(name):
    return _mesh()[0] if name == "mesh" else _disks2()[0]


def _pods(t, kw, laws=None, energy=None):
    """(spec, laws, energy or None) as the raw entry points take them; `keep` holds what they point to"""
    spec, _, keep = t._pathsSpec("test", kw.get("sticking"), kw.get("reflectivity"), kw["reflection"], kw["maxBounces"], 1.0, True)
    laws = laws or {}
    lpod, keepLaws = t._angularLaws("test", laws.get("sourceLaw"), laws.get("reflectivityLaw"), laws.get("yieldLaw"))
    epod = keepEnergy = None
    if energy is not None:
        epod, keepEnergy = t._energyTables("test", energy.get("energyYield"), energy.get("energyMax"), energy.get("sourceEnergy"),
                                           energy.get("sourceQuantiles"), energy.get("retentionLaw"), energy.get("energyCut", True))
    return spec, lpod, epod, (keep, keepLaws, keepEnergy)


def _ref(p):
    return C.byref(p) if p is not None else None


# ---------------------------------------------------------------------------------------------------------------
# 1. the three identities, for the fixed-K, sums, adaptive and one-path forms
# ---------------------------------------------------------------------------------------------------------------
def _all_forms(t, samples, laws, energy, kw):
    """(flux, sum, sumSq, adaptive flux, adaptive samples, the first paths' (end, throughput, weight)) of one setting;
    energy: a dict of gatherEnergy's keywords, "null" (the raw entry points with energy == NULL) or None (gatherAngular)"""
    if isinstance(energy, dict):
        flux = t.gatherEnergy(samples, numpy=True, **laws, **energy, **kw)
        s1, s2 = t.gatherEnergySums(0, 1, samples, numpy=True, **laws, **energy, **kw)
        af, _, au = t.gatherEnergyAdaptive(0.2, minSamples=64, maxSamples=256, numpy=True, **laws, **energy, **kw)
        paths = [t.debugGatherEnergyPath(7, k, energy, laws=laws, **kw) for k in range(4)]
    elif energy is None:
        flux = t.gatherAngular(samples, numpy=True, **laws, **kw)
        s1, s2 = t.gatherAngularSums(0, 1, samples, numpy=True, **laws, **kw)
        af, _, au = t.gatherAngularAdaptive(0.2, minSamples=64, maxSamples=256, numpy=True, **laws, **kw)
        paths = [t.debugGatherAngularPath(7, k, laws=laws, **kw) for k in range(4)]
    else:
        n = int(t._L.vr_num_primitives(t._h))
        spec, lpod, _, keep = _pods(t, kw, laws)
        flux, s1, s2 = np.empty(n, np.float32), np.empty(n, np.int64), np.empty(n, np.int64)
        fp = C.POINTER(C.c_float)
        t._check(t._L.vr_gather_energy(t._h, C.byref(spec), C.byref(lpod), None, 0, n, samples, flux.ctypes.data_as(fp)))
        t._check(t._L.vr_gather_energy_sums(t._h, C.byref(spec), C.byref(lpod), None, 0, n, 0, 1, samples, s1.ctypes.data_as(I64),
                                            s2.ctypes.data_as(I64)))
        af, err, au = np.empty(n, np.float32), np.empty(n, np.float32), np.empty(n, np.uint32)
        info = capi.GatherAdaptiveInfoPOD()
        t._check(t._L.vr_gather_energy_adaptive(t._h, C.byref(spec), C.byref(lpod), None, 0, n, 64, 256, 0.2, 0.0, af.ctypes.data_as(fp),
                                                err.ctypes.data_as(fp), au.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(info)))
        paths = []
        for k in range(4):
            count, end = C.c_uint32(0), C.c_uint32(0)
            T, w = C.c_float(0.0), C.c_float(0.0)
            e4 = np.full(4, -5.0, np.float32)
            t._check(t._L.vr_debug_gather_energy_path(t._h, C.byref(spec), C.byref(lpod), None, 7, k, 0, None, None, C.byref(count),
                                                      C.byref(end), None, C.byref(T), C.byref(w), e4.ctypes.data_as(fp)))
            assert (e4 == -5.0).all()  # (energy == NULL: the angular call, energyOut left alone)
            paths.append(dict(numVertices=count.value, end=end.value, throughput=np.float32(T.value), weight=np.float32(w.value)))
    tails = [(p["numVertices"], p["end"], int(_bits(p["throughput"])[0]), int(_bits(p["weight"])[0])) for p in paths]
    return _bits(flux), s1, s2, _bits(af), np.asarray(au, dtype=np.int64), tails


def _same(a, b, what):
    for x, y, name in zip(a[:5], b[:5], ("flux", "sum", "sumSq", "adaptive flux", "adaptive samples")):
        assert np.array_equal(x, y), (what, name)
    assert a[5] == b[5], (what, "paths")


@pytest.mark.parametrize("scene", ["mesh", "disks2"])
@pytest.mark.parametrize("samples", [64, 100])
def test_identities_with_gather_angular(scene, samples):
    t = _scene(scene)
    laws = dict(reflectivityLaw=R5, yieldLaw=Y5)
    for kind in KINDS:
        kw = dict(reflectivity=0.8, reflection=kind, maxBounces=8)
        want = _all_forms(t, samples, laws, None, kw)
        assert (want[1] > 0).any()
        # energy == NULL
        _same(_all_forms(t, samples, laws, "null", kw), want, (scene, samples, kind, "energy NULL"))
        # an all-ones yield of any M, with anything in the other fields
        for M in (2, 256):
            ones = dict(energyYield=np.ones(M, np.float32), energyMax=3.5, sourceQuantiles=Q3, retentionLaw=EPS)
            _same(_all_forms(t, samples, laws, ones, kw), want, (scene, samples, kind, "all ones", M))
        ones = dict(energyYield=np.ones(5, np.float32), energyMax=100.0, sourceEnergy=250.0, energyCut=False)
        _same(_all_forms(t, samples, laws, ones, kw), want, (scene, samples, kind, "all ones, monoenergetic"))
        # sticking 0, no yield law, sourceEnergy = energyMax = 1, energyYield {0, 1}, retentionLaw R: reflectivityLaw R
        kw0 = dict(sticking=0.0, reflection=kind, maxBounces=8)
        for R in (R5, np.array([0.0, 0.5, 1.0], np.float32)):  # (the second absorbs some paths: T = 0 there, e = 0 here)
            want0 = _all_forms(t, samples, dict(reflectivityLaw=R), None, kw0)
            got0 = _all_forms(t, samples, {}, dict(energyYield=[0.0, 1.0], energyMax=1.0, sourceEnergy=1.0, retentionLaw=R), kw0)
            assert (want0[1] > 0).any()
            for x, y, name in zip(got0[:5], want0[:5], ("flux", "sum", "sumSq", "adaptive flux", "adaptive samples")):
                assert np.array_equal(x, y), (scene, samples, kind, "retention is the reflectivity law", name)
            # (the one-path walk's T is 1 here and the law's there: the weights are the same, and the ends unless absorbed)
            assert [p[3] for p in got0[5]] == [p[3] for p in want0[5]]


# ---------------------------------------------------------------------------------------------------------------
# 2. the cut changes no bit, and it does cut
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["mesh", "disks2"])
@pytest.mark.parametrize("samples", [64, 100])
def test_cut_on_is_cut_off_bit_for_bit(scene, samples):
    t = _scene(scene)
    for kind in KINDS:
        kw = dict(reflectivity=0.8, reflection=kind, maxBounces=8)
        on = _all_forms(t, samples, {}, dict(ION, energyCut=True), kw)
        off = _all_forms(t, samples, {}, dict(ION, energyCut=False), kw)
        for x, y, name in zip(on[:5], off[:5], ("flux", "sum", "sumSq", "adaptive flux", "adaptive samples")):
            assert np.array_equal(x, y), (scene, samples, kind, name)
        assert (on[1] > 0).any()
        assert [p[3] for p in on[5]] == [p[3] for p in off[5]]  # the weights; the ends differ where the cut fired


def test_the_cut_fires_and_some_samples_are_never_walked():
    t, g, _ = _mesh()
    prims = (int(np.nonzero(g.part == cf.BOTTOM)[0][3]), int(np.nonzero(g.part == cf.LEFT)[0][11]))
    fired = unwalked = shorter = 0
    for kind in KINDS:
        kw = dict(reflectivity=0.8, reflection=kind, maxBounces=8)
        for prim in prims:
            for k in range(64):
                on = t.debugGatherEnergyPath(prim, k, dict(ION, energyCut=True), **kw)
                off = t.debugGatherEnergyPath(prim, k, dict(ION, energyCut=False), **kw)
                assert off["end"] != vr.GatherEnd.ENERGY and _bits(on["weight"])[0] == _bits(off["weight"])[0]
                assert _bits(on["u"])[0] == _bits(off["u"])[0] and _bits(on["E0"])[0] == _bits(off["E0"])[0]
                if on["end"] == vr.GatherEnd.ENERGY:
                    fired += 1
                    assert on["weight"] == 0 and on["numVertices"] <= off["numVertices"]
                    assert law(YE, on["e"]) == 0 and on["e"] * np.float32(2) < 1  # xs = 2 e < Z0 - 1 = 1
                    unwalked += int(on["numVertices"] == 1)
                    shorter += int(on["numVertices"] < off["numVertices"])
                    if on["numVertices"] == 1:
                        assert on["P"] == 1 and on["E0"] < 50
                else:
                    assert on["numVertices"] == off["numVertices"] and on["end"] == off["end"]
    print("the cut ended %d of 256 paths, %d before their walk, %d shorter than without it" % (fired, unwalked, shorter))
    assert fired > 20 and unwalked > 5 and shorter > 5 and fired > unwalked


# ---------------------------------------------------------------------------------------------------------------
# 3. paths replayed multiply by multiply
# ---------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    """vdot / gather_dot of the library in float32: (x x + y y) + z z"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.float32(np.float32(np.float32(a[0] * b[0]) + np.float32(a[1] * b[1])) + np.float32(a[2] * b[2]))


def _cut(e, M, Z0):
    xs = np.float32(np.minimum(np.maximum(np.float32(e), np.float32(0)), np.float32(1)) * np.float32(M - 1))
    return bool(xs < np.float32(Z0 - 1))


def _replay(p, prim, sample, rho, max_bounces, cut):
    """u, E0, every eps(mu), P, e, T and the weight of one recorded path from its vertices alone, in float32"""
    u = energy_u([SEED], [prim], [sample])[0]
    E0 = law(Q3, u)
    P, T, bounces, ended, end = ONE, ONE, 0, False, None
    e = np.float32(np.float32(E0 * P) / np.float32(100.0))
    v = len(p["ids"])
    looked = 0
    if cut and _cut(e, 3, 2):
        assert v == 1 and p["numVertices"] == 1
        ended, end = True, vr.GatherEnd.ENERGY
    for k in range(1, v):
        assert not ended
        front = float((p["arriving"][k].astype(np.float32) * p["normals"][k]).astype(np.float32).sum(dtype=np.float64)) < 0
        if not front or bounces >= max_bounces:
            ended = True
            break
        T = np.float32(T * rho)
        assert not np.isnan(p["leaving"][k]).any()  # (R5 > 0: no path is absorbed; the cut's last vertex keeps its direction)
        mu = _dot(p["normals"][k], p["leaving"][k])
        assert -1e-6 <= mu <= 1 + 1e-6
        T = np.float32(T * law(R5, mu))
        P = np.float32(P * law(EPS, mu))
        looked += 1
        e = np.float32(np.float32(E0 * P) / np.float32(100.0))
        if cut and _cut(e, 3, 2):  # the rule, after the update of P: the path ends on this vertex
            assert k == v - 1
            ended, end = True, vr.GatherEnd.ENERGY
            break
        assert k < v - 1 or p["end"] != vr.GatherEnd.ENERGY
        bounces += 1
    w = np.float32(0)
    if not ended and p["end"] == vr.GatherEnd.MISS and p["direction"][2] > 0:  # u = +z; power 1: g c^0 = 1
        w = np.float32(np.float32(ONE * T) * law(YE, e))
    if end is not None:
        assert p["end"] == end
    assert _bits(u)[0] == _bits(p["u"])[0] and _bits(E0)[0] == _bits(p["E0"])[0]
    assert _bits(P)[0] == _bits(p["P"])[0] and _bits(e)[0] == _bits(p["e"])[0], (P, p["P"], e, p["e"])
    assert _bits(T)[0] == _bits(p["throughput"])[0] and _bits(w)[0] == _bits(p["weight"])[0], (T, p["throughput"], w, p["weight"])
    return w, looked


def _q(weights, budget):
    w = np.minimum(np.asarray(weights, dtype=np.float32), np.float32(2.0 ** 22 / budget))
    return int(np.where(w > 0, (w.astype(np.float64) * 2.0 ** 40 + 0.5).astype(np.int64), 0).sum())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cut", [True, False])
def test_paths_replayed_multiply_by_multiply(kind, cut):
    t, g, _ = _mesh()
    prims = (int(np.nonzero(g.part == cf.TOP)[0][5]), int(np.nonzero(g.part == cf.LEFT)[0][11]),
             int(np.nonzero(g.part == cf.BOTTOM)[0][3]))
    energy = dict(ION, energyCut=cut)
    kw = dict(reflectivity=0.8, reflection=kind, maxBounces=8)
    looked = reached = 0
    for prim in prims:
        ws = []
        for k in range(64):
            p = t.debugGatherEnergyPath(prim, k, energy, laws=dict(reflectivityLaw=R5), **kw)
            assert p["ids"][0] == prim
            w, n = _replay(p, prim, k, np.float32(0.8), 8, cut)
            ws.append(w)
            looked += n
            reached += int(w > 0)
        s1, _ = t.gatherEnergySums(0, 1, 64, primFirst=prim, primCount=1, numpy=True, reflectivityLaw=R5, **energy, **kw)
        assert int(s1[0]) == _q(ws, 64), (prim, int(s1[0]))
    print("%s cut %s: %d retention look-ups replayed, %d paths weigh something" % (kind.name, cut, looked, reached))
    assert looked > 20 and reached > 20


# ---------------------------------------------------------------------------------------------------------------
# 4. - 6. range splits, entry points, the adaptive call
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_same_bits_over_ranges_and_entry_points(kind):
    import torch
    t, g, _ = _mesh()
    n = len(g.tris)
    kw = dict(reflectivity=0.8, reflection=kind, maxBounces=8, reflectivityLaw=R5, yieldLaw=Y5, **ION)
    whole = t.gatherEnergy(100, numpy=True, **kw)
    angular = t.gatherAngular(100, numpy=True, reflectivity=0.8, reflection=kind, maxBounces=8, reflectivityLaw=R5, yieldLaw=Y5)
    assert (whole > 0).any() and (whole <= angular).all() and (whole < angular).any()  # (Y_E <= 1)
    first = 200  # a range of 65 primitives: one call, and 1 + 64
    r65 = t.gatherEnergy(100, primFirst=first, primCount=65, numpy=True, **kw)
    parts = np.concatenate([t.gatherEnergy(100, primFirst=a, primCount=b, numpy=True, **kw) for a, b in ((first, 1), (first + 1, 64))])
    assert (_bits(r65) == _bits(whole[first:first + 65])).all() and (_bits(parts) == _bits(r65)).all()
    dev = t.gatherEnergy(100, **kw)  # the device entry point
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and (_bits(dev.cpu().numpy()) == _bits(whole)).all()
    dev65 = t.gatherEnergy(100, primFirst=first, primCount=65, **kw)
    assert (_bits(dev65.cpu().numpy()) == _bits(r65)).all()
    kwt = dict(kw)
    del kwt["reflectivity"]
    table = t.gatherEnergy(100, sticking=torch.full((n,), 0.2, device="cuda"), **kwt)
    assert isinstance(table, torch.Tensor) and (_bits(table.cpu().numpy()) == _bits(whole)).all()  # (1 - 0.2f == 0.8f)
    s1, s2 = t.gatherEnergySums(0, 1, 64, numpy=True, **kw)
    d1, d2 = t.gatherEnergySums(0, 1, 64, **kw)
    assert (d1.cpu().numpy() == s1).all() and (d2.cpu().numpy() == s2).all()
    assert (_bits((s1.astype(np.float64) / 2.0 ** 40 / 64).astype(np.float32)) == _bits(t.gatherEnergy(64, numpy=True, **kw))).all()
    assert t.gatherEnergy(100, primFirst=5, primCount=0, numpy=True, **kw).shape == (0,)


@pytest.mark.parametrize("scene", ["mesh", "disks2"])
def test_adaptive_flux_has_the_bits_of_the_fixed_call_at_its_count(scene):
    import torch
    t = _scene(scene)
    kw = dict(reflectivity=0.8, reflection=GR.DIFFUSE, maxBounces=8, reflectivityLaw=R5, **ION)
    flux, err, used, info = t.gatherEnergyAdaptive(0.15, minSamples=64, maxSamples=512, returnInfo=True, numpy=True, **kw)
    print("%s: primitives by samples used %s" % (scene, dict(zip(*(a.tolist() for a in np.unique(used, return_counts=True))))))
    assert set(np.unique(used)) <= {64, 128, 256, 512} and len(np.unique(used)) > 1 and info["totalSamples"] == int(used.sum())
    for k in np.unique(used):
        fixed = t.gatherEnergy(int(k), numpy=True, **kw)
        sel = used == k
        assert (_bits(flux[sel]) == _bits(fixed[sel])).all(), (scene, int(k))
    assert (err[flux > 0] > 0).any()
    dflux, derr, dused = t.gatherEnergyAdaptive(0.15, minSamples=64, maxSamples=512, **kw)
    assert isinstance(dflux, torch.Tensor) and (_bits(dflux.cpu().numpy()) == _bits(flux)).all()
    assert (_bits(derr.cpu().numpy()) == _bits(err)).all() and (dused.cpu().numpy() == used.astype(np.int32)).all()


# ---------------------------------------------------------------------------------------------------------------
# 7. a closed form that goes through no other gather
# ---------------------------------------------------------------------------------------------------------------
def test_direct_flux_times_the_mean_yield_per_triangle():
    """sticking 1, a power-1 source, sourceQuantiles {0, energyMax}, energyYield [0, 0, 1]: energy and direction are
    independent, E[Y_E] = int_1/2^1 (2 e - 1) de = 1/4, so every triangle's flux is its direct flux / 4.  Weights lie in
    [0, 1]: sigma^2 = F (1 - F) / K.  (tests/test_gather_energy_host.py runs the same estimator in numpy against the same
    reference and bound)"""
    t, g, coord = _mesh()
    K = 4096
    out = t.gatherEnergy(K, energyYield=YE, energyMax=100.0, sourceQuantiles=[0.0, 100.0], sticking=1.0, maxBounces=0, numpy=True)
    inside = g.part != cf.TOP
    F = np.ones(len(g.tris))
    F[inside] = cf.radiosity(cf.W, cf.DEPTH, 1.0).direct_at(g.part[inside], coord[inside])[0]
    F = F / 4.0
    bound = 5.0 * np.sqrt(F * (1.0 - F) / K)
    err = np.abs(out.astype(np.float64) - F)
    k = int(np.argmax(err / bound))
    print("direct / 4: %d triangles, worst uses %.0f %% of its bound (got %.5f ref %.5f bound %.5f)"
          % (len(F), 100 * err[k] / bound[k], out[k], F[k], bound[k]))
    bad = np.nonzero(~(err <= bound))[0]
    assert len(bad) == 0, [(int(q), float(out[q]), float(F[q]), float(bound[q])) for q in bad[:10]]
    assert (F[inside] < 0.2).all() and (out[g.part == cf.BOTTOM] > 0).all()


# ---------------------------------------------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------------------------------------------
def _energy(yield_=None, quantiles=None, retention=None, counts=None, energyMax=100.0, sourceEnergy=50.0, cut=1):
    keep = [None if a is None else np.ascontiguousarray(a, dtype=np.float32) for a in (yield_, quantiles, retention)]
    pod = capi.GatherEnergyPOD(energyMax=energyMax, sourceEnergy=sourceEnergy, energyCut=cut)
    for k, (field, count) in enumerate((("energyYield", "energyYieldCount"), ("sourceQuantiles", "sourceQuantilesCount"),
                                        ("retentionLaw", "retentionCount"))):
        if keep[k] is not None:
            setattr(pod, field, keep[k].ctypes.data)
            setattr(pod, count, keep[k].size if counts is None else counts[k])
    pod.keep = keep  # (the tables live as long as the struct that points to them)
    return pod


def test_refusals_leave_out_untouched_and_the_context_usable():
    import torch
    t, g, _ = _mesh()
    n = len(g.tris)
    poison = np.float32(-123.5)
    kw = dict(reflectivity=0.8, maxBounces=5, reflectivityLaw=R5, **ION)
    want = t.gatherEnergy(64, numpy=True, **kw)
    spec = capi.GatherSpecPOD(cosinePower=1.0, mode=0, paths=1, reflection=0, maxBounces=5, reflectivityScalar=0.8)
    nan, inf = float("nan"), float("inf")
    big = np.ones(300, np.float32)
    fp = C.POINTER(C.c_float)

    def raw(spec, laws, energy, first, count, samples, out):
        return t._L.vr_gather_energy(t._h, _ref(spec), _ref(laws), _ref(energy), first, count, samples,
                                     out.ctypes.data_as(fp) if out is not None else None)

    cases = [  # (energy, samples, a word of the message)
        (_energy(), 64, b"energyYield must not be null"),
        (_energy(yield_=big, counts=(1, 0, 0)), 64, b"energyYield must have 2 .. 256"),
        (_energy(yield_=big, counts=(257, 0, 0)), 64, b"energyYield must have 2 .. 256"),
        (_energy(yield_=YE, quantiles=big, counts=(3, 300, 0)), 64, b"sourceQuantiles must have 2 .. 256"),
        (_energy(yield_=YE, retention=big, counts=(3, 0, 1)), 64, b"retentionLaw must have 2 .. 256"),
        (_energy(yield_=[0.0, 1.0, -0.5, nan]), 64, b"energyYield[2]"),
        (_energy(yield_=[0.0, inf]), 64, b"energyYield[1]"),
        (_energy(yield_=YE, quantiles=[1.0, 2.0, 3.0, -1.0, nan]), 64, b"sourceQuantiles[3]"),
        (_energy(yield_=YE, quantiles=[nan, 2.0]), 64, b"sourceQuantiles[0]"),
        (_energy(yield_=YE, retention=[0.5, 1.0, 1.5, -1.0]), 64, b"retentionLaw[2]"),
        (_energy(yield_=YE, retention=[0.5, nan]), 64, b"retentionLaw[1]"),
        (_energy(yield_=YE, energyMax=0.0), 64, b"energyMax"),
        (_energy(yield_=YE, energyMax=-1.0), 64, b"energyMax"),
        (_energy(yield_=YE, energyMax=inf), 64, b"energyMax"),
        (_energy(yield_=YE, energyMax=nan), 64, b"energyMax"),
        (_energy(yield_=YE, sourceEnergy=-1.0), 64, b"sourceEnergy"),
        (_energy(yield_=YE, sourceEnergy=inf), 64, b"sourceEnergy"),
        (_energy(yield_=YE, sourceEnergy=nan), 64, b"sourceEnergy"),
        (_energy(yield_=YE, cut=2), 64, b"energyCut is 0 or 1"),
        (_energy(yield_=[0.0, 2.0]), 1 << 22, b"wbound"),      # samples x max Y_E = 2^23
        (_energy(yield_=YE), (1 << 22) + 1, b"2^22"),          # what vr_gather_angular refuses: samples x g
    ]
    for energy, samples, word in cases:
        out = np.full(n, poison, np.float32)
        assert raw(spec, None, energy, 0, n, samples, out) == capi.VR_E_INVALID, word
        assert (out == poison).all() and word in t._L.vr_last_error(t._h), (word, t._L.vr_last_error(t._h))
    # the angular yield counts in wbound: max Y x max Y_E = 3 x 2 at 2^20 samples
    ylaw = capi.GatherLawsPOD()
    ykeep = np.ascontiguousarray(Y5)
    ylaw.yieldLaw, ylaw.yieldCount = ykeep.ctypes.data, ykeep.size
    out = np.full(n, poison, np.float32)
    assert raw(spec, ylaw, _energy(yield_=[0.0, 2.0]), 0, n, 1 << 20, out) == capi.VR_E_INVALID and b"wbound" in t._L.vr_last_error(t._h)
    # a negative sourceEnergy is not read where there are quantiles
    assert raw(spec, None, _energy(yield_=YE, quantiles=Q3, sourceEnergy=-1.0), 0, n, 64, out) == capi.VR_OK
    # what the angular call refuses: its laws, its spec, the range, a null out
    bad_law = capi.GatherLawsPOD()
    bkeep = np.array([0.5, 1.5], np.float32)
    bad_law.reflectivityLaw, bad_law.reflectivityCount = bkeep.ctypes.data, 2
    out = np.full(n, poison, np.float32)
    assert raw(spec, bad_law, _energy(yield_=YE), 0, n, 64, out) == capi.VR_E_INVALID and b"reflectivityLaw[1]" in t._L.vr_last_error(t._h)
    for bad in (None, capi.GatherSpecPOD(cosinePower=1.0, paths=0), capi.GatherSpecPOD(cosinePower=1.0, paths=1, mode=1),
                capi.GatherSpecPOD(cosinePower=1.0, paths=1, reflection=2), capi.GatherSpecPOD(cosinePower=1.0, paths=1, reflectivityScalar=1.5),
                capi.GatherSpecPOD(cosinePower=1.0, paths=1, maxBounces=65536)):
        assert raw(bad, None, _energy(yield_=YE), 0, n, 64, out) == capi.VR_E_INVALID and (out == poison).all()
    assert raw(spec, None, _energy(yield_=YE), 1, n, 64, out) == capi.VR_E_INVALID and (out == poison).all()  # the range
    assert raw(spec, None, _energy(yield_=YE), 0, n, 64, None) == capi.VR_E_INVALID  # out null
    assert raw(spec, None, _energy(yield_=[-1.0, 1.0]), 0, 0, 64, None) == capi.VR_E_INVALID  # the tables are checked first
    assert raw(spec, None, _energy(yield_=YE), 0, 0, 64, None) == capi.VR_OK  # nothing to do, after the checks
    # the sums, the adaptive call and the one-path walk refuse the same tables
    with pytest.raises(vr.VrError, match=r"retentionLaw\[1\]"):
        t.gatherEnergySums(0, 1, 64, energyYield=YE, energyMax=1.0, sourceEnergy=1.0, retentionLaw=[0.5, 2.0], reflectivity=0.8, numpy=True)
    with pytest.raises(vr.VrError, match=r"energyYield\[0\]"):
        t.gatherEnergyAdaptive(0.05, energyYield=[-1.0, 2.0], energyMax=1.0, sourceEnergy=1.0, reflectivity=0.8)
    with pytest.raises(vr.VrError, match="wbound"):
        t.gatherEnergyAdaptive(0.05, energyYield=[1.0, 2.0], energyMax=1.0, sourceEnergy=1.0, reflectivity=0.8, minSamples=1 << 21,
                               maxSamples=1 << 22)
    with pytest.raises(vr.VrError, match="energyMax"):
        t.debugGatherEnergyPath(0, 0, dict(energyYield=YE, energyMax=0.0, sourceEnergy=1.0), reflectivity=0.8)
    with pytest.raises(ValueError):
        t.debugGatherEnergyPath(0, 0, dict(energyYield=YE, energyMax=1.0, sourceEnergy=1.0, spread=0.1), reflectivity=0.8)
    with pytest.raises(ValueError):
        t.gatherEnergy(64, energyYield=YE, energyMax=1.0, sourceEnergy=1.0, sourceQuantiles=Q3, reflectivity=0.8)
    with pytest.raises(ValueError):
        t.gatherEnergy(64, energyMax=1.0, sourceEnergy=1.0, reflectivity=0.8)  # no yield
    # the device form refuses host memory for out, and leaves device memory as it was on a refused table
    host = np.full(n, poison, np.float32)
    dev = torch.full((n,), float(poison), device="cuda")
    L = t._L
    ok, bad = _energy(yield_=YE), _energy(yield_=[1.0, -2.0])
    assert L.vr_gather_energy_device(t._h, C.byref(spec), None, C.byref(ok), 0, n, 64, C.c_void_p(host.ctypes.data), None) == capi.VR_E_INVALID
    assert L.vr_gather_energy_device(t._h, C.byref(spec), None, C.byref(bad), 0, n, 64, C.c_void_p(dev.data_ptr()), None) == capi.VR_E_INVALID
    torch.cuda.synchronize()
    assert (host == poison).all() and bool((dev == float(poison)).all())
    # ... and the context still answers
    assert (_bits(t.gatherEnergy(64, numpy=True, **kw)) == _bits(want)).all()


# ---------------------------------------------------------------------------------------------------------------
# 9. an apply is untouched
# ---------------------------------------------------------------------------------------------------------------
def _apply_twice(gather_between):
    g = cf.trench_mesh()
    t = _mesh_tracer(g)
    t.setParticleType(vr.DiffuseParticle(0.3, "flux"))
    t.setNumberOfRaysFixed(200_000)
    t.setRngSeed(SEED)
    t.setUseRandomSeeds(False)
    t.apply()
    first = np.array(t.getLocalData().getVectorData("flux"))
    if gather_between:
        t.gatherEnergy(128, reflectivity=0.8, numpy=True, reflectivityLaw=R5, **ION)
        t.gatherEnergy(64, sticking=np.full(len(g.tris), 0.2, np.float32), reflection=GR.DIFFUSE, yieldLaw=Y5, **ION)
        t.gatherEnergyAdaptive(0.1, reflectivity=0.8, maxSamples=256, **ION)
        t.gatherEnergySums(0, 1, 64, reflectivity=0.8, **ION)
        t.debugGatherEnergyPath(5, 3, ION, reflectivity=0.8)
        with pytest.raises(vr.VrError):
            t.gatherEnergy(64, reflectivity=0.8, energyYield=[-1.0, 1.0], energyMax=1.0, sourceEnergy=1.0)
        assert (_bits(t.getLocalData().getVectorData("flux")) == _bits(first)).all()
    t.apply()
    return first, np.array(t.getLocalData().getVectorData("flux")), t.getRayTraceInfo().as_dict()


def test_an_apply_is_untouched_by_an_energy_gather():
    f0, s0, i0 = _apply_twice(False)
    f1, s1, i1 = _apply_twice(True)
    assert (_bits(f0) == _bits(f1)).all() and (_bits(s0) == _bits(s1)).all()
    skip = {"time", "timeBuild", "timeTrace", "timeTraceKernel", "timeGenKernel"}
    assert {k: v for k, v in i0.items() if k not in skip} == {k: v for k, v in i1.items() if k not in skip}


# ---------------------------------------------------------------------------------------------------------------
# 10. the C++ façade
# ---------------------------------------------------------------------------------------------------------------
def test_cpp_facade_gather_energy(tmp_path):
    """tests/aux/facade_gather_energy.cpp on a sheet of disks folded into V grooves; the values it prints are the Python
    call's on the same scene, bit for bit"""
    flags = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include",
             "-I", os.path.join(ROOT, "include", "viennaray_amd"), "-I", os.path.join(ROOT, "include")]
    src = os.path.join(ROOT, "tests", "aux", "facade_gather_energy.cpp")
    exe = tmp_path / "facade_gather_energy"
    lib = os.path.join(ROOT, "viennaray_amd")
    subprocess.check_call(["g++", "-O1"] + flags + [src, "-o", str(exe), "-L", lib, "-lviennaray_amd",
                                                    "-L", "/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib,
                                                    "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "facade gather energy ok" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    printed = {line.split()[0]: np.array([float.fromhex(v) for v in line.split()[1:]], np.float32)
               for line in out.stdout.splitlines() if line.startswith("ion")}
    import math
    n = 16
    pts, nrm = [], []
    for i in range(n):
        for j in range(n):
            k = i % 8
            s = -1.0 if k < 4 else 1.0
            pts.append((float(i), float(j), 1.5 * abs(k - 4)))
            nrm.append((-s * 1.5 / math.sqrt(3.25), 0.0, 1.0 / math.sqrt(3.25)))
    t = vr.TraceDisk(3)
    t.setGeometry(np.array(pts, np.float32), np.array(nrm, np.float32), 1.0)
    t.setBoundaryConditions([BC.PERIODIC_BOUNDARY] * 3)
    t.setParticleType(vr.DiffuseParticle(0.3, "flux"))
    t.setNumberOfRaysFixed(20000)
    t.setUseRandomSeeds(False)
    t.setRngSeed(7)
    t.applyPrepare()
    want = t.gatherEnergy(256, energyYield=[0.0, 0.0, 0.0, 0.5, 1.0], energyMax=100.0, sourceQuantiles=[40.0, 80.0, 100.0],
                          retentionLaw=[1.0, 0.3], reflectivityLaw=[1.0, 0.8, 0.6, 0.4, 0.2], yieldLaw=[0.5, 3.0], sticking=0.2,
                          maxBounces=8, numpy=True)
    assert (want > 0).any() and (_bits(printed["ion"]) == _bits(want)).all()
