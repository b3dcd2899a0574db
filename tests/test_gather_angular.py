"""gatherAngular on the device (vr_gather_angular*, vr_debug_gather_angular_path; Trace.gatherAngular,
gatherAngularAdaptive, gatherAngularSums, debugGatherAngularPath): gatherPaths weighed by tabulated angular laws — the
source's radiance L(c), the reflectivity R(mu) by the cosine of incidence, the yield Y(mu0) by the sample's own starting
angle.  Bit identities with gatherPaths / gatherFlux (no law, all-ones laws, R = 0.5, Y = 2), same bits over range
splits, entry points and the adaptive call, single paths replayed in numpy float32 look-up by look-up, three closed forms
per triangle (tests/angular_forms.py: quadratures derived from neither the oracle nor the library), the refusals, and an
apply left as it was.  The scenes are those of tests/test_gather_paths.py, re-created here."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import viennaray_amd as vr
from viennaray_amd import capi
import angular_forms as af
import closed_forms as cf
from test_gather_angular_host import np_law

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BC = vr.BoundaryCondition
GR = vr.GatherReflection
SEED = 7
K = 4096
ONE = np.float32(1.0)
KINDS = [GR.SPECULAR, GR.DIFFUSE]
# the laws of the replay: M = 5, R falling from 1 at mu = 0 to 0.2 at mu = 1, Y rising from 0.5 to 3, L sampled from c^3
R5 = np.linspace(1.0, 0.2, 5).astype(np.float32)
Y5 = np.linspace(0.5, 3.0, 5).astype(np.float32)
L5 = (np.linspace(0.0, 1.0, 5) ** 3).astype(np.float32)


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


@functools.lru_cache(maxsize=None)
def _flat():
    n = 16
    i, j = np.meshgrid(np.arange(n, dtype=np.float32), np.arange(n, dtype=np.float32), indexing="ij")
    pts = np.stack([i.ravel(), j.ravel(), np.zeros(n * n, np.float32)], 1)
    nrm = np.tile(np.array([0, 0, 1], np.float32), (n * n, 1))
    t = vr.TraceDisk(3)
    t.setGeometry(pts, nrm, 1.0)
    t.setBoundaryConditions([BC.PERIODIC_BOUNDARY] * 3)
    return _prepared(t)


def _scene(name):
    return _mesh()[0] if name == "mesh" else _disks2()[0]


def _check(name, got, ref, bound):
    got, ref, bound = (np.asarray(a, dtype=np.float64) for a in (got, ref, bound))
    err = np.abs(got - ref)
    k = int(np.argmax(err / bound))
    print("%s: %d primitives, worst uses %.0f %% of its bound (got %.5f ref %.5f bound %.5f)"
          % (name, len(got), 100 * err[k] / bound[k], got[k], ref[k], bound[k]))
    bad = np.nonzero(~(err <= bound))[0]
    assert len(bad) == 0, [(int(q), float(got[q]), float(ref[q]), float(bound[q])) for q in bad[:10]]


def _bd(F, g, k=K):
    """5 sigma of a mean of k samples in [0, g] with expectation F (Bhatia-Davis: var <= F (g - F))"""
    F = np.asarray(F, dtype=np.float64)
    return 5.0 * np.sqrt(np.clip(F * (g - F), 0.0, None) / k) + 1e-5


def _result(weights, samples):
    """q(), the int64 sum and gather_result of vr_gather.hpp in numpy"""
    w = np.minimum(np.asarray(weights, dtype=np.float32), np.float32(2.0 ** 22 / samples))  # (samples: a power of two here)
    q = np.where(w > 0, (w.astype(np.float64) * 2.0 ** 40 + 0.5).astype(np.int64), 0)
    return np.float32(float(q.sum()) / 2.0 ** 40 / samples)


# ---------------------------------------------------------------------------------------------------------------
# 1. bit identities
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["mesh", "disks2"])
@pytest.mark.parametrize("samples", [64, 100])
def test_no_law_is_gather_paths_and_no_bounce_is_gather_flux(scene, samples):
    t = _scene(scene)
    flux = t.gatherFlux(samples, numpy=True)
    assert (flux > 0).any() and (flux < 1).any()
    for kind in KINDS:
        kw = dict(reflectivity=0.8, reflection=kind, maxBounces=5, numpy=True)
        want = t.gatherPaths(samples, **kw)
        assert (want > flux).any()  # (something bounced)
        assert (_bits(t.gatherAngular(samples, **kw)) == _bits(want)).all(), (scene, samples, kind)
        none = t.gatherAngular(samples, reflectivity=0.8, reflection=kind, maxBounces=0, numpy=True)
        assert (_bits(none) == _bits(flux)).all(), (scene, samples, kind)
        # ... and with laws that cannot act without a bounce or are 1
        same = t.gatherAngular(samples, reflectivityLaw=R5, yieldLaw=np.ones(3, np.float32), reflectivity=0.8, reflection=kind,
                               maxBounces=0, numpy=True)
        assert (_bits(same) == _bits(flux)).all(), (scene, samples, kind)


@pytest.mark.parametrize("scene", ["mesh", "disks2"])
@pytest.mark.parametrize("samples", [64, 100])
@pytest.mark.parametrize("M", [2, 256])
def test_all_ones_laws_are_gather_paths(scene, samples, M):
    """g_L of an all-ones source law is exactly 1.0f in both dimensions, and a look-up in a constant table is the constant"""
    t = _scene(scene)
    ones = np.ones(M, np.float32)
    for kind in KINDS:
        kw = dict(reflectivity=0.8, reflection=kind, maxBounces=5, numpy=True)
        want = t.gatherPaths(samples, **kw)
        got = t.gatherAngular(samples, sourceLaw=ones, reflectivityLaw=ones, yieldLaw=ones, **kw)
        assert (_bits(got) == _bits(want)).all(), (scene, samples, M, kind)
        for one in (dict(sourceLaw=ones), dict(reflectivityLaw=ones), dict(yieldLaw=ones), dict(stickingLaw=np.zeros(M, np.float32))):
            assert (_bits(t.gatherAngular(samples, **one, **kw)) == _bits(want)).all(), (scene, samples, M, kind, list(one))


@pytest.mark.parametrize("scene", ["mesh", "disks2"])
@pytest.mark.parametrize("samples", [64, 100])
def test_half_reflectivity_law_is_half_the_reflectivity(scene, samples):
    """(T * 0.8f) * 0.5f and T * 0.4f are the same float: 0.4f is 0.8f / 2 and a power of two commutes with the rounding"""
    t = _scene(scene)
    assert np.float32(0.8) * np.float32(0.5) == np.float32(0.4)
    for kind in KINDS:
        want = t.gatherPaths(samples, reflectivity=0.4, reflection=kind, maxBounces=5, numpy=True)
        got = t.gatherAngular(samples, reflectivityLaw=np.full(7, 0.5, np.float32), reflectivity=0.8, reflection=kind, maxBounces=5,
                              numpy=True)
        assert (_bits(got) == _bits(want)).all(), (scene, samples, kind)
        assert (want > t.gatherFlux(samples, numpy=True)).any()


@pytest.mark.parametrize("scene", ["mesh", "disks2"])
@pytest.mark.parametrize("budget", [64, 100])
def test_a_yield_of_two_doubles_the_sums(scene, budget):
    """the first chunk of a call of 64 and of 100 samples.  q(2 w) = 2 q(w) exactly where w 2^40 is an integer: with at most
    8 bounces w = T >= 0.8^8 > 2^-3 has its last bit at 2^-26 or above, and 2 w stays below wmax.  The squares: q2(2 w) =
    4 q2(w) where w^2 2^28 is an integer or rounds alike; only the first sums are compared exactly"""
    t = _scene(scene)
    for kind in KINDS:
        kw = dict(reflectivity=0.8, reflection=kind, maxBounces=8, numpy=True)
        s1, s2 = t.gatherPathsSums(0, 1, budget, **kw)
        a1, a2 = t.gatherAngularSums(0, 1, budget, yieldLaw=np.full(4, 2.0, np.float32), **kw)
        assert s1.dtype == np.int64 and (s1 > 0).any()
        assert (a1 == 2 * s1).all(), (scene, budget, kind)
        assert (np.abs(a2 - 4 * s2) <= 2 * 64).all()  # (a square is rounded at 2^-28: each of 64 samples within 2 units)
        n1, n2 = t.gatherAngularSums(0, 1, budget, **kw)
        assert (n1 == s1).all() and (n2 == s2).all()


# ---------------------------------------------------------------------------------------------------------------
# 2. same bits for splits, entry points and the adaptive call
# ---------------------------------------------------------------------------------------------------------------
LAWS = dict(sourceLaw=L5, reflectivityLaw=R5, yieldLaw=Y5)


@pytest.mark.parametrize("kind", KINDS)
def test_same_bits_over_ranges_and_entry_points(kind):
    import torch
    t, g, _ = _mesh()
    n = len(g.tris)
    kw = dict(reflectivity=0.8, reflection=kind, maxBounces=5, **LAWS)
    whole = t.gatherAngular(100, numpy=True, **kw)
    assert (whole > 0).any() and (_bits(whole) != _bits(t.gatherPaths(100, reflectivity=0.8, reflection=kind, maxBounces=5,
                                                                       numpy=True))).any()
    first = 200  # a range of 65 primitives: one call, and 1 + 64
    r65 = t.gatherAngular(100, primFirst=first, primCount=65, numpy=True, **kw)
    parts = np.concatenate([t.gatherAngular(100, primFirst=a, primCount=b, numpy=True, **kw) for a, b in ((first, 1), (first + 1, 64))])
    assert (_bits(r65) == _bits(whole[first:first + 65])).all() and (_bits(parts) == _bits(r65)).all()
    dev = t.gatherAngular(100, **kw)  # the device entry point
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and (_bits(dev.cpu().numpy()) == _bits(whole)).all()
    dev65 = t.gatherAngular(100, primFirst=first, primCount=65, **kw)
    assert (_bits(dev65.cpu().numpy()) == _bits(r65)).all()
    table = t.gatherAngular(100, sticking=torch.full((n,), 0.2, device="cuda"), reflection=kind, maxBounces=5, **LAWS)
    assert isinstance(table, torch.Tensor) and (_bits(table.cpu().numpy()) == _bits(whole)).all()  # (1 - 0.2f == 0.8f)
    host = t.gatherAngular(100, reflectivity=np.full(n, 0.8, np.float32), reflection=kind, maxBounces=5, **LAWS)
    assert isinstance(host, np.ndarray) and (_bits(host) == _bits(whole)).all()
    as_tensor = t.gatherAngular(100, numpy=True, reflectivity=0.8, reflection=kind, maxBounces=5, sourceLaw=torch.from_numpy(L5).cuda(),
                                stickingLaw=(ONE - R5).astype(np.float32), yieldLaw=list(map(float, Y5)))
    assert (_bits(as_tensor) == _bits(t.gatherAngular(100, numpy=True, reflectivity=0.8, reflection=kind, maxBounces=5, sourceLaw=L5,
                                                        reflectivityLaw=(ONE - (ONE - R5)).astype(np.float32), yieldLaw=Y5))).all()
    assert t.gatherAngular(100, primFirst=5, primCount=0, numpy=True, **kw).shape == (0,)


@pytest.mark.parametrize("scene", ["mesh", "disks2"])
def test_adaptive_flux_has_the_bits_of_the_fixed_call_at_its_count(scene):
    import torch
    t = _scene(scene)
    kw = dict(reflectivity=0.8, reflection=GR.DIFFUSE, maxBounces=5, **LAWS)
    # (15 %: the flat top, whose weights spread by 0.85 of their mean, stops at 64 samples; the shadowed primitives go on)
    flux, err, used, info = t.gatherAngularAdaptive(0.15, minSamples=64, maxSamples=512, returnInfo=True, numpy=True, **kw)
    print("%s: primitives by samples used %s" % (scene, dict(zip(*(a.tolist() for a in np.unique(used, return_counts=True))))))
    assert set(np.unique(used)) <= {64, 128, 256, 512} and len(np.unique(used)) > 1 and info["totalSamples"] == int(used.sum())
    for k in np.unique(used):
        fixed = t.gatherAngular(int(k), numpy=True, **kw)
        sel = used == k
        assert (_bits(flux[sel]) == _bits(fixed[sel])).all(), (scene, int(k))
    assert (err[flux > 0] > 0).any()
    dflux, derr, dused = t.gatherAngularAdaptive(0.15, minSamples=64, maxSamples=512, **kw)
    assert isinstance(dflux, torch.Tensor) and (_bits(dflux.cpu().numpy()) == _bits(flux)).all()
    assert (_bits(derr.cpu().numpy()) == _bits(err)).all() and (dused.cpu().numpy() == used.astype(np.int32)).all()
    # the sums over the first chunk divide to the fixed call, host and device
    s1, _ = t.gatherAngularSums(0, 1, 64, numpy=True, **kw)
    d1, _ = t.gatherAngularSums(0, 1, 64, **kw)
    assert (d1.cpu().numpy() == s1).all()
    assert (_bits((s1.astype(np.float64) / 2.0 ** 40 / 64).astype(np.float32)) == _bits(t.gatherAngular(64, numpy=True, **kw))).all()


# ---------------------------------------------------------------------------------------------------------------
# 3. one path, replayed
# ---------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    """vdot / gather_dot of the library in float32: (x x + y y) + z z"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.float32(np.float32(np.float32(a[0] * b[0]) + np.float32(a[1] * b[1])) + np.float32(a[2] * b[2]))


def _replay(p, rho, max_bounces, gL):
    """T and the weight of one recorded path from its vertices alone: every mu, every look-up, every multiply in float32"""
    v = len(p["ids"])
    T, bounces, ended = ONE, 0, False
    looked = 0
    for k in range(1, v):
        front = float((p["arriving"][k].astype(np.float32) * p["normals"][k]).astype(np.float32).sum(dtype=np.float64)) < 0
        if not front or bounces >= max_bounces:
            ended = True
            break
        T = np.float32(T * rho)
        assert T != 0 and not np.isnan(p["leaving"][k]).any()
        mu = _dot(p["normals"][k], p["leaving"][k])
        assert -1e-6 <= mu <= 1 + 1e-6  # (the look-up clamps what rounding leaves outside [0, 1])
        T = np.float32(T * np_law(R5, mu))
        looked += 1
        bounces += 1
    assert ended == bool(np.isnan(p["leaving"][v - 1]).any())
    c_end = p["direction"][2]  # u = +z
    w = np.float32(0)
    if not ended and p["end"] == capi.VR_GATHER_END_MISS and c_end > 0:
        mu0 = _dot(p["normals"][0], p["leaving"][0])
        w = np.float32(np.float32(np.float32(gL * np_law(L5, c_end)) * T) * np_law(Y5, mu0))
    assert _bits(T)[0] == _bits(p["throughput"])[0] and _bits(w)[0] == _bits(p["weight"])[0], (T, p["throughput"], w, p["weight"])
    return w, looked


@pytest.mark.parametrize("kind", KINDS)
def test_paths_replayed_look_up_by_look_up(kind):
    t, g, _ = _mesh()
    gL = np.float32(np.pi / af.norm3(L5))  # the normalisation by an independent quadrature; exact for a piecewise-linear law
    prims = (int(np.nonzero(g.part == cf.BOTTOM)[0][3]), int(np.nonzero(g.part == cf.LEFT)[0][11]),
             int(np.nonzero(g.part == cf.RIGHT)[0][150]))
    looked = reached = 0
    for prim in prims:
        kw = dict(reflectivity=0.8, reflection=kind, maxBounces=48)
        paths = [t.debugGatherAngularPath(prim, k, laws=LAWS, **kw) for k in range(64)]
        plain = [t.debugGatherPath(prim, k, **kw) for k in range(64)]
        ws = []
        for p, q in zip(paths, plain):
            # the laws weigh the path, they do not move it (R5 > 0: no path is absorbed)
            assert p["numVertices"] == q["numVertices"] and p["end"] == q["end"] and (_bits(p["leaving"][:-1]) == _bits(q["leaving"][:-1])).all()
            assert p["ids"][0] == prim
            w, n = _replay(p, np.float32(0.8), 48, gL)
            ws.append(w)
            looked += n
            reached += int(w > 0)
        got = t.gatherAngular(64, primFirst=prim, primCount=1, numpy=True, **LAWS, **kw)
        assert _bits(got)[0] == _bits(_result(ws, 64))[0], (prim, got)
    print("%s: %d reflectivity look-ups replayed, %d paths reached the source" % (kind.name, looked, reached))
    assert looked > 100 and reached > 30


# ---------------------------------------------------------------------------------------------------------------
# 4. closed forms per triangle
# ---------------------------------------------------------------------------------------------------------------
def _unique(fn, coord):
    """fn over the distinct coordinates (the centroids of a row of triangles share theirs), spread back"""
    u, inv = np.unique(coord, return_inverse=True)
    return fn(u)[inv]


def _source_law(n=3, M=33):
    c = np.linspace(0.0, 1.0, M)
    return (c ** (n - 1) * (1 + c) / 2).astype(np.float32)


def test_source_law_on_the_bottom_per_triangle():
    """sticking 1, no bounce, L = the table of c^2 (1 + c) / 2 at M = 33: (1 / Z) iint L(cos phi cos psi) cos phi cos^2 psi over
    the opening, at every bottom centroid.  Weights lie in [0, g_L max L]"""
    t, g, coord = _mesh()
    L = _source_law()
    out = t.gatherAngular(K, sourceLaw=L, sticking=1.0, maxBounces=0, numpy=True)
    b = g.part == cf.BOTTOM
    F, diff = af.converged(lambda x, n: _unique(lambda u: af.source_bottom(L, u, n), x), coord[b], n=128)
    assert diff <= 1e-6
    wbound = np.pi / af.norm3(L) * float(L.max())
    assert 2.0 < wbound < 2.5
    _check("source law, bottom", out[b], F, _bd(F, wbound))
    # the flat top sees the whole source: int L c d omega / Z = 1
    top = g.part == cf.TOP
    _check("source law, top", out[top], np.ones(top.sum()), _bd(np.ones(top.sum()), wbound))


def test_source_law_on_the_2d_bottom_per_disk():
    """the 2-D trench: int L(cos phi) cos phi d phi / Z_2 over the opening, at every bottom disk"""
    t, g = _disks2()
    L = _source_law()
    out = t.gatherAngular(K, sourceLaw=L, sticking=1.0, maxBounces=0, numpy=True)
    b = g.part == cf.BOTTOM
    F, diff = af.converged(lambda x, n: af.source_bottom_2d(L, x, n), g.coord[b], n=256)
    assert diff <= 1e-6
    wbound = 2.0 / af.norm2(L) * float(L.max())
    _check("source law, 2-D bottom", out[b], F, _bd(F, wbound))


def test_yield_law_on_the_walls_per_triangle():
    """a power-1 source, sticking 1, Y(mu) = 0.5 + 2.5 mu: on a wall mu0 = sin phi cos psi is NOT c — a kernel that looked Y up
    at c would pass on the bottom and fail here.  Weights lie in [0, max Y]"""
    t, g, coord = _mesh()
    Y = np.array([0.5, 3.0], np.float32)
    out = t.gatherAngular(K, yieldLaw=Y, sticking=1.0, maxBounces=0, numpy=True)
    walls = (g.part == cf.LEFT) | (g.part == cf.RIGHT)
    F, diff = af.converged(lambda z, n: _unique(lambda u: af.yield_wall(Y, u, n), z), coord[walls], n=32)
    assert diff <= 1e-6
    unit = _unique(lambda u: af.yield_wall(np.ones(2), u, 32), coord[walls])
    assert np.abs(unit - af.yield_wall_unit(coord[walls])).max() < 1e-12  # Y = 1: (1 - cos phi_max) / 2
    wrong = _unique(lambda u: af.yield_wall(Y, u, 32, look_up_at_c=True), coord[walls])  # a kernel that took c for mu0
    assert (np.abs(F - wrong) > 1.5 * _bd(F, 3.0)).sum() >= walls.sum() // 4  # (it would miss there by half a bound or more)
    _check("yield law, walls", out[walls], F, _bd(F, 3.0))


def test_reflectivity_law_on_the_bottom_per_triangle():
    """SPECULAR, rho = 0.8, a power-1 source, R(mu) = 1 - 0.8 mu: the image sum of closed_forms.specular_bottom with
    (rho R(|sin phi| cos psi))^|k| inside the direction integral of image k.  Weights lie in [0, 1]; paths cut at B bounces
    lack at most 0.8^(B + 1)"""
    t, g, coord = _mesh()
    R = np.array([1.0, 0.2], np.float32)
    B = 64
    out = t.gatherAngular(K, reflectivityLaw=R, reflectivity=0.8, reflection=GR.SPECULAR, maxBounces=B, numpy=True)
    b = g.part == cf.BOTTOM
    F, diff = af.converged(lambda x, n: _unique(lambda u: af.reflectivity_bottom(R, 0.8, u, n), x), coord[b], n=16)
    assert diff <= 1e-6
    plain = cf.specular_bottom(cf.W, cf.DEPTH, 0.2, coord[b])
    assert (plain - F > 0.05).all()  # (the law takes a good part of what the walls reflect)
    _check("reflectivity law, bottom", out[b], F, _bd(F, 1.0) + 0.8 ** (B + 1))


# ---------------------------------------------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------------------------------------------
def _raw(t, spec, laws, first, count, samples, out):
    fp = C.POINTER(C.c_float)
    return t._L.vr_gather_angular(t._h, C.byref(spec) if spec is not None else None, C.byref(laws) if laws is not None else None,
                                  first, count, samples, out.ctypes.data_as(fp) if out is not None else None)


def _laws(source=None, reflectivity=None, yield_=None, counts=None):
    keep = [None if a is None else np.ascontiguousarray(a, dtype=np.float32) for a in (source, reflectivity, yield_)]
    pod = capi.GatherLawsPOD()
    for k, (field, count) in enumerate((("sourceLaw", "sourceCount"), ("reflectivityLaw", "reflectivityCount"), ("yieldLaw", "yieldCount"))):
        if keep[k] is not None:
            setattr(pod, field, keep[k].ctypes.data)
            setattr(pod, count, keep[k].size if counts is None else counts[k])
    pod.keep = keep  # (the tables live as long as the struct that points to them)
    return pod, keep


def test_refusals_leave_out_untouched_and_the_context_usable():
    import torch
    t, g, _ = _mesh()
    n = len(g.tris)
    poison = np.float32(-123.5)
    kw = dict(reflectivity=0.8, maxBounces=5, **LAWS)
    want = t.gatherAngular(64, numpy=True, **kw)
    spec = capi.GatherSpecPOD(cosinePower=1.0, mode=0, paths=1, reflection=0, maxBounces=5, reflectivityScalar=0.8)
    nan, inf = float("nan"), float("inf")
    big = np.ones(300, np.float32)
    cases = [  # (laws, samples, a word of the message)
        (_laws(source=big, counts=(1, 0, 0)), 64, b"sourceLaw must have 2 .. 256"),
        (_laws(reflectivity=big, counts=(0, 257, 0)), 64, b"reflectivityLaw must have 2 .. 256"),
        (_laws(yield_=big, counts=(0, 0, 0)), 64, b"yieldLaw must have 2 .. 256"),
        (_laws(source=[1.0, 0.5, -0.25, nan]), 64, b"sourceLaw[2]"),
        (_laws(source=[1.0, inf]), 64, b"sourceLaw[1]"),
        (_laws(source=[0.0, 0.0, 0.0]), 64, b"sourceLaw must not be 0 everywhere"),
        (_laws(reflectivity=[0.5, 1.0, 1.5, -1.0]), 64, b"reflectivityLaw[2]"),
        (_laws(reflectivity=[nan, 0.5]), 64, b"reflectivityLaw[0]"),
        (_laws(yield_=[1.0, 2.0, 3.0, -0.5, nan]), 64, b"yieldLaw[3]"),
        (_laws(yield_=[1.0, inf]), 64, b"yieldLaw[1]"),
        (_laws(yield_=[1.0, 2.0]), 1 << 22, b"wbound"),            # samples x max Y = 2^23
        (_laws(yield_=[0.5, 1.0]), (1 << 22) + 1, b"2^22"),        # what vr_gather_paths refuses: samples x g
        (_laws(source=[0.0, 0.0, 0.0, 1.0]), 1 << 21, b"wbound"),  # a narrow source law: g_L max L = 27 / 8
    ]
    for (laws, keep), samples, word in cases:
        out = np.full(n, poison, np.float32)
        assert _raw(t, spec, laws, 0, n, samples, out) == capi.VR_E_INVALID, word
        assert (out == poison).all() and word in t._L.vr_last_error(t._h), (word, t._L.vr_last_error(t._h))
    # a source law takes the place of the power cosine
    spec8 = capi.GatherSpecPOD(cosinePower=8.0, mode=0, paths=1, reflection=0, maxBounces=5, reflectivityScalar=0.8)
    out = np.full(n, poison, np.float32)
    assert _raw(t, spec8, _laws(source=L5)[0], 0, n, 64, out) == capi.VR_E_INVALID and b"cosinePower must be 1" in t._L.vr_last_error(t._h)
    assert _raw(t, spec8, _laws(yield_=Y5)[0], 0, n, 64, out) == capi.VR_OK  # (the other laws go with any power)
    assert (_bits(out) == _bits(t.gatherAngular(64, yieldLaw=Y5, reflectivity=0.8, maxBounces=5, cosinePower=8.0, numpy=True))).all()
    # the spec: paths 1, NORMAL, no emission; what vr_gather_paths refuses
    emission = np.zeros(n, np.float32)
    for bad in (None, capi.GatherSpecPOD(cosinePower=1.0, paths=0), capi.GatherSpecPOD(cosinePower=1.0, paths=1, mode=1),
                capi.GatherSpecPOD(cosinePower=1.0, paths=1, emission=emission.ctypes.data),
                capi.GatherSpecPOD(cosinePower=1.0, paths=1, reflection=2), capi.GatherSpecPOD(cosinePower=0.5, paths=1),
                capi.GatherSpecPOD(cosinePower=1.0, paths=1, reflectivityScalar=1.5),
                capi.GatherSpecPOD(cosinePower=1.0, paths=1, maxBounces=65536)):
        out = np.full(n, poison, np.float32)
        assert _raw(t, bad, _laws(yield_=Y5)[0], 0, n, 64, out) == capi.VR_E_INVALID and (out == poison).all()
        assert _raw(t, bad, None, 0, n, 64, out) == capi.VR_E_INVALID and (out == poison).all()
    out = np.full(n, poison, np.float32)
    assert _raw(t, spec, _laws(yield_=Y5)[0], 1, n, 64, out) == capi.VR_E_INVALID and (out == poison).all()  # the range
    assert _raw(t, spec, _laws(yield_=Y5)[0], 0, n, 64, None) == capi.VR_E_INVALID  # out null
    assert _raw(t, spec, _laws(yield_=[-1.0, 1.0])[0], 0, 0, 64, None) == capi.VR_E_INVALID  # the laws are checked first
    assert _raw(t, spec, _laws(yield_=Y5)[0], 0, 0, 64, None) == capi.VR_OK  # nothing to do, after the checks
    assert _raw(t, spec, None, 0, n, 64, out) == capi.VR_OK  # laws NULL: no law
    assert (_bits(out) == _bits(t.gatherPaths(64, reflectivity=0.8, maxBounces=5, numpy=True))).all()
    # the sums, the adaptive call and the one-path walk refuse the same laws
    with pytest.raises(vr.VrError, match=r"reflectivityLaw\[1\]"):
        t.gatherAngularSums(0, 1, 64, reflectivityLaw=[0.5, 2.0], reflectivity=0.8, numpy=True)
    with pytest.raises(vr.VrError, match=r"yieldLaw\[0\]"):
        t.gatherAngularAdaptive(0.05, yieldLaw=[-1.0, 2.0], reflectivity=0.8)
    with pytest.raises(vr.VrError, match="wbound"):
        t.gatherAngularAdaptive(0.05, yieldLaw=[1.0, 2.0], reflectivity=0.8, minSamples=1 << 21, maxSamples=1 << 22)
    with pytest.raises(vr.VrError, match=r"sourceLaw\[0\]"):
        t.debugGatherAngularPath(0, 0, laws=dict(sourceLaw=[-1.0, 2.0]), reflectivity=0.8)
    with pytest.raises(ValueError):
        t.debugGatherAngularPath(0, 0, laws=dict(coneLaw=[1.0, 2.0]), reflectivity=0.8)
    with pytest.raises(ValueError):
        t.gatherAngular(64, reflectivityLaw=R5, stickingLaw=R5, reflectivity=0.8)
    with pytest.raises(ValueError):
        t.gatherAngular(64, yieldLaw=Y5)  # neither sticking nor reflectivity
    # the device form refuses host memory for out, and leaves device memory as it was on a refused law
    host = np.full(n, poison, np.float32)
    dev = torch.full((n,), float(poison), device="cuda")
    L = t._L
    ok, keep = _laws(yield_=Y5)
    assert L.vr_gather_angular_device(t._h, C.byref(spec), C.byref(ok), 0, n, 64, C.c_void_p(host.ctypes.data), None) == capi.VR_E_INVALID
    bad, keep2 = _laws(yield_=[1.0, -2.0])
    assert L.vr_gather_angular_device(t._h, C.byref(spec), C.byref(bad), 0, n, 64, C.c_void_p(dev.data_ptr()), None) == capi.VR_E_INVALID
    torch.cuda.synchronize()
    assert (host == poison).all() and bool((dev == float(poison)).all())
    # ... and the context still answers
    assert (_bits(t.gatherAngular(64, numpy=True, **kw)) == _bits(want)).all()


def test_an_angular_gather_needs_what_a_prepare_left():
    g = cf.trench_mesh()
    t = _mesh_tracer(g)
    t.setParticleType(vr.DiffuseParticle(1.0, "flux"))
    t.setNumberOfRaysFixed(1000)
    t.setRngSeed(SEED)
    with pytest.raises(vr.VrError, match="nothing to gather from"):
        t.gatherAngular(64, reflectivity=0.8, numpy=True, **LAWS)
    with pytest.raises(vr.VrError, match="nothing to gather from"):
        t.debugGatherAngularPath(0, 0, laws=LAWS, reflectivity=0.8)
    t.setMaxBoundaryHits(1 << 16)
    t.applyPrepare()
    want = _mesh()[0].gatherAngular(64, reflectivity=0.8, maxBounces=5, numpy=True, **LAWS)
    assert (_bits(t.gatherAngular(64, reflectivity=0.8, maxBounces=5, numpy=True, **LAWS)) == _bits(want)).all()


def test_flat_surface_weighs_what_the_laws_say():
    """a flat sheet under the source: every sample reaches it, mu0 = c, no vertex: the flux is the mean of g_L L(c) Y(c) over
    the sheet's own samples, the same for every disk up to its engine — and exactly Y's constant for a constant yield"""
    t = _flat()
    out = t.gatherAngular(128, yieldLaw=np.full(9, 2.5, np.float32), reflectivity=0.8, numpy=True)
    assert out.shape == (256,) and (_bits(out) == _bits(np.float32(2.5))).all()


# ---------------------------------------------------------------------------------------------------------------
# 6. an apply is untouched
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
        t.gatherAngular(128, reflectivity=0.8, numpy=True, **LAWS)
        t.gatherAngular(64, sticking=np.full(len(g.tris), 0.2, np.float32), reflection=GR.DIFFUSE, yieldLaw=Y5, cosinePower=8.0)
        t.gatherAngularAdaptive(0.1, reflectivity=0.8, maxSamples=256, **LAWS)
        t.gatherAngularSums(0, 1, 64, reflectivity=0.8, **LAWS)
        t.debugGatherAngularPath(5, 3, laws=LAWS, reflectivity=0.8)
        with pytest.raises(vr.VrError):
            t.gatherAngular(64, reflectivity=0.8, yieldLaw=[-1.0, 1.0])
        assert (_bits(t.getLocalData().getVectorData("flux")) == _bits(first)).all()
    t.apply()
    return first, np.array(t.getLocalData().getVectorData("flux")), t.getRayTraceInfo().as_dict()


def test_an_apply_is_untouched_by_an_angular_gather():
    f0, s0, i0 = _apply_twice(False)
    f1, s1, i1 = _apply_twice(True)
    assert (_bits(f0) == _bits(f1)).all() and (_bits(s0) == _bits(s1)).all()
    skip = {"time", "timeBuild", "timeTrace", "timeTraceKernel", "timeGenKernel"}
    assert {k: v for k, v in i0.items() if k not in skip} == {k: v for k, v in i1.items() if k not in skip}


# ---------------------------------------------------------------------------------------------------------------
# 7. the C++ façade
# ---------------------------------------------------------------------------------------------------------------
def test_cpp_facade_gather_angular(tmp_path):
    """tests/aux/facade_gather_angular.cpp on a sheet of disks folded into V grooves; the values it prints are the Python
    call's on the same scene, bit for bit"""
    flags = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include",
             "-I", os.path.join(ROOT, "include", "viennaray_amd"), "-I", os.path.join(ROOT, "include")]
    src = os.path.join(ROOT, "tests", "aux", "facade_gather_angular.cpp")
    exe = tmp_path / "facade_gather_angular"
    lib = os.path.join(ROOT, "viennaray_amd")
    subprocess.check_call(["g++", "-O1"] + flags + [src, "-o", str(exe), "-L", lib, "-lviennaray_amd",
                                                    "-L", "/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib,
                                                    "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "facade gather angular ok" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    printed = {line.split()[0]: np.array([float.fromhex(v) for v in line.split()[1:]], np.float32)
               for line in out.stdout.splitlines() if line.startswith("mixed")}
    import math
    n = 16
    pts, nrm = [], []
    for i in range(n):
        for j in range(n):
            k = i % 8
            s = -1.0 if k < 4 else 1.0
            pts.append([float(i), float(j), 1.5 * abs(k - 4)])
            nrm.append([-s * 1.5 / math.sqrt(3.25), 0.0, 1.0 / math.sqrt(3.25)])
    t = vr.TraceDisk(3)
    t.setGeometry(np.array(pts, np.float32), np.array(nrm, np.float32), 1.0)
    t.setBoundaryConditions([BC.PERIODIC_BOUNDARY] * 3)
    _prepared(t)
    got = t.gatherAngular(256, sourceLaw=[0.0, 0.125, 1.0], reflectivityLaw=[1.0, 0.8, 0.6, 0.4, 0.2], yieldLaw=[0.5, 3.0], sticking=0.2,
                          maxBounces=8, numpy=True)
    assert printed["mixed"].shape == got.shape and (_bits(printed["mixed"]) == _bits(got)).all()
