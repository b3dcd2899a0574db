"""Edge-case rays (tests/edge_rays.py) against the oracle's BRUTE FORCE on every path that decides a closest hit:
the two per-lane walks through vr_debug_intersect, and — as host rays, one family to a launch, so that whole waves are
made of one kind of ray — the packet walk, the packet query with its scene-box clip and wall pre-test, and the
LDS-resident small-scene kernel inside apply().  Then the ordinary source on scenes moved far from the origin, where the
box padding and the height field's pad have to scale with the coordinates.

Every one of those paths is an exact primitive test (hit_disc, hit_tri, the tie rule: min t, boundary first, lower
original id) behind a conservative cull; the tests here sit on the margins of the culls.  A failure prints the ray as hex
floats, so that it reproduces as one ray in test_debug_intersect_equals_brute_force."""
import functools

import numpy as np
import pytest

import viennaray_amd as vr
from viennaray_amd import TraceDirection as TD
from oracle import pyoracle as po
from helpers import l2_rel
import edge_rays as er

pytestmark = pytest.mark.gpu

INFO_KEYS = ("numRays", "totalRaysTraced", "nonGeometryHits", "geometryHits", "particleHits",
             "boundaryHits", "reflections", "raysTerminated")
STICKINGS = (1.0, 0.3)


def info_dict(t):
    i = t.getRayTraceInfo()
    return {k: int(getattr(i, k)) for k in INFO_KEYS}


# ---------------------------------------------------------------------------------------------------------------
# (a) the per-lane walks, ray by ray
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _debug_tracer(scene):
    t = er.new_tracer(scene)
    t.setParticleType(vr.DiffuseParticle(1.0, "f"))
    return t


def _assert_same_hits(o, d, got, ref, what):
    g, p, t = got
    g0, p0, t0 = ref
    bad = np.flatnonzero((g != g0) | ((g0 >= 0) & ((p != p0) | (t.view(np.uint32) != t0.view(np.uint32)))))
    if bad.size:
        i = bad[0]
        pytest.fail("%s: %d of %d rays differ; first is ray %d: %s\n  brute force: geom %d prim %d t %s\n  device:      "
                    "geom %d prim %d t %s" % (what, bad.size, len(g), i, er.hexray(o[i], d[i]), g0[i], p0[i],
                                              float(t0[i]).hex(), g[i], p[i], float(t[i]).hex()))


DEBUG_CELLS = [(s, f, w) for s in er.SCENES for f in er.family_names(s) for w in ("0", "1")]
DEBUG_CELLS += [(er.KNOWN_ANSWERS[k][0], k, w) for k in sorted(er.KNOWN_ANSWERS) for w in ("0", "1")]


@pytest.mark.parametrize("scene,family,walk", DEBUG_CELLS, ids=["%s-%s-walk%s" % c for c in DEBUG_CELLS])
def test_debug_intersect_equals_brute_force(scene, family, walk, monkeypatch):
    """vr_debug_intersect (default tnear 1e-4) under the escape-link walk (VR_DEBUG_WALK=0) and the ordered pair walk (=1):
    geomID, primID and the bits of t of the oracle's brute force, on all families — and on the single rays that once
    exposed a fault (edge_rays.KNOWN_ANSWERS), which stay when the families are reseeded."""
    if family in er.KNOWN_ANSWERS:
        o, d, ref = er.known_answer(family)
    else:
        o, d = er.scene_families(scene)[family]
        ref = er.reference(scene, family)
    monkeypatch.setenv("VR_DEBUG_WALK", walk)
    got = _debug_tracer(scene).debugIntersect(o, d)
    _assert_same_hits(o, d, got, ref, "%s/%s walk %s" % (scene, family, walk))


# ---------------------------------------------------------------------------------------------------------------
# (b), (c) host rays through apply()
# ---------------------------------------------------------------------------------------------------------------
def _host_rays(scene, family):
    """(origins, directions, maxBoundaryHits); family "all": every source-side family concatenated"""
    fams = er.scene_families(scene)
    if family == "all":
        names = er.source_side_names(scene)
        return (np.concatenate([fams[f][0] for f in names]), np.concatenate([fams[f][1] for f in names]), 1000)
    return fams[family][0], fams[family][1], er.max_boundary_hits(family)


def _host_tracer(scene, sticking, o, d, max_bh):
    s = er.scene(scene)
    t = er.new_tracer(scene)
    t.setBoundaryConditions(er.boundary_conditions(s.D))
    t.setParticleType(vr.DiffuseParticle(sticking, "flux"))
    t.setMaxBoundaryHits(max_bh)
    t.setRngSeed(5)
    t.setHostRays(o, d)
    return t


def _host_oracle(scene, sticking, o, d, max_bh):
    s = er.scene(scene)
    orc = er.new_oracle(scene)
    orc.set_boundary_conditions([int(b) for b in er.boundary_conditions(s.D)])
    orc.set_particle(po.DIFFUSE, sticking)
    orc.set_max_boundary_hits(max_bh)
    orc.set_rng_seed(5)
    orc.set_host_rays(o, d)
    orc.set_lazy_rng(True)
    return orc


def _blame(scene, sticking, o, d, max_bh, f, r):
    """the first primitive whose flux differs, and the rays the oracle credited to it (event log of a single-threaded
    re-run): each of them reproduces the fault as one ray of test_debug_intersect_equals_brute_force"""
    k = int(np.flatnonzero(f != r)[0])
    orc = _host_oracle(scene, sticking, o, d, max_bh)
    orc.set_event_capacity(64 * len(o) + 4096)
    orc.apply(1)
    ev = orc.events()
    near = {k}
    if er.scene(scene).verts is None:
        near |= {int(j) for j in orc.neighbors(k)}  # (a disk is also credited through a hit of an overlapping neighbour)
    rays = sorted({int(i) for i, kind, p in zip(ev["ray"], ev["kind"], ev["prim"]) if kind == 3 and int(p) in near})
    lines = ["first differing primitive %d: device %r oracle %r; %d oracle rays credited it:" % (k, float(f[k]), float(r[k]), len(rays))]
    lines += ["  ray %d: %s" % (i, er.hexray(o[i], d[i])) for i in rays[:12]]
    return "\n".join(lines)


HOST_CELLS = [(s, st, f) for s in er.SCENES for st in STICKINGS for f in er.source_side_names(s) + ("all",)]


@pytest.mark.parametrize("scene,sticking,family", HOST_CELLS, ids=["%s-%s-%s" % c for c in HOST_CELLS])
def test_host_rays_through_apply(scene, sticking, family):
    """One family ALONE as host rays (no draws, no weights): every wave holds 64 rays of that one kind — in a mixture a
    grazing ray among 63 ordinary ones would be a straggler that the packet paths hand to the per-lane walk.  Sticking 1
    runs the absorbing kernels, 0.3 the general ones.  Counters equal the oracle's, flux bit-equal (integer sums) or within
    the suite's bound for "same rays, other summation order"."""
    o, d, max_bh = _host_rays(scene, family)
    t = _host_tracer(scene, sticking, o, d, max_bh)
    orc = _host_oracle(scene, sticking, o, d, max_bh)
    t.apply()
    orc.apply(po.max_threads())
    assert t.traceMode() == er.MODES[scene][sticking], t.traceMode()
    oi = orc.info()
    assert not oi["warning"] and not oi["error"]
    f, r = np.asarray(t.getLocalData().getVectorData(0)), orc.flux()
    gi = info_dict(t)
    print(scene, sticking, family, gi, "l2_rel", l2_rel(f, r))
    same = (f == r).all() if sticking >= 1.0 else l2_rel(f, r) <= 5e-6
    if not same:
        pytest.fail("flux differs (l2_rel %.3e, counters %r, oracle %r)\n%s" % (
            l2_rel(f, r), gi, {k: oi[k] for k in INFO_KEYS}, _blame(scene, sticking, o, d, max_bh, f, r)))
    assert gi == {k: oi[k] for k in INFO_KEYS}
    assert gi["numRays"] == len(o) and gi["geometryHits"] >= len(o) // 10


PATH_KNOBS = [
    {"VR_DEBUG_FLAGS": "32"},                       # no packets
    {"VR_DEBUG_FLAGS": "128"},                      # no packet query
    {"VR_PACKET_BUDGET": "0"},
    {"VR_PQ_CAND": "63", "VR_PQ_FRONTIER": "64"},   # queries run to the end
    {"VR_PQ_CAND": "2"},                            # ... or give up half way
    {"VR_PQ_MARGIN": "0"},                          # no frontier cache
    {"VR_SMALL_SCENE": "0"},                        # small scenes from HBM
    {"VR_WALK_PARK": "1"},
    {"VR_HOST_BUILD": "1"},                         # the host's BVH builder
]
PATH_CELLS = [(s, st) for s in er.SCENES for st in STICKINGS]


@pytest.mark.parametrize("scene,sticking", PATH_CELLS, ids=["%s-%s" % c for c in PATH_CELLS])
def test_host_rays_same_bits_on_every_path(scene, sticking, monkeypatch):
    """The concatenated set and the grazing set again with the packet paths, the packet query, the small-scene kernel and
    the device builder switched off or pushed to their extremes: identical accumulator bits and counters.  Together with
    test_host_rays_through_apply this tells WHICH path is wrong when one is."""
    for family in ("all", "graze"):
        o, d, max_bh = _host_rays(scene, family)

        def run():
            t = _host_tracer(scene, sticking, o, d, max_bh)
            t.apply()
            return t.getFluxF64(), info_dict(t), t.traceMode()

        f0, i0, m0 = run()
        assert m0 == er.MODES[scene][sticking], m0
        assert i0["geometryHits"] >= len(o) // 10
        for knobs in PATH_KNOBS:
            with monkeypatch.context() as m:
                for k, v in knobs.items():
                    m.setenv(k, v)
                f, i, mode = run()
            assert i == i0, (family, knobs, mode)
            assert (f == f0).all(), (family, knobs, mode, int(np.flatnonzero(f != f0)[0]))


# ---------------------------------------------------------------------------------------------------------------
# (d) scenes far from the origin
# ---------------------------------------------------------------------------------------------------------------
def _rippled_surface(n=120, gd=0.5, amp=0.5, wave=2.0):
    """A gently rippled sheet of disks (z = amp sin(x / wave) cos(y / wave), normals of the height field): flat with
    relief, the scene of the relief modes (5 absorbing / 6 general)."""
    ax = (np.arange(n) - (n - 1) / 2.0) * gd
    x, y = np.meshgrid(ax, ax, indexing="ij")
    z = amp * np.sin(x / wave) * np.cos(y / wave)
    nx = -amp / wave * np.cos(x / wave) * np.cos(y / wave)
    ny = amp / wave * np.sin(x / wave) * np.sin(y / wave)
    nrm = np.stack([nx, ny, np.ones_like(nx)], -1).reshape(-1, 3)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    pts = np.stack([x, y, z], -1).reshape(-1, 3)
    return pts.astype(np.float32), nrm.astype(np.float32), gd


FAR_MODES = {"plane": {1.0: 1, 0.3: 3}, "ripple": {1.0: 5, 0.3: 6}, "trench3d": {1.0: 2, 0.3: 0}, "trench2d": {1.0: 4, 0.3: 4}}
FAR_CELLS = [(s, st) for s in FAR_MODES for st in STICKINGS]


@pytest.mark.parametrize("scene,sticking", FAR_CELLS, ids=["%s-%s" % c for c in FAR_CELLS])
def test_scenes_far_from_the_origin(scene, sticking):
    """The ordinary source on scenes translated (in float32) by (+2048, -1024, +512): the box padding (4e-6 of the scale)
    and the height field's pad (1e-5 of it) scale with the largest coordinate on purpose, and here they have to.  The
    translated float32 arrays ARE the scene, for the device and the oracle alike.  This is also the only route by which
    edge conditions reach the relief modes (5 / 6): the relief bins are filled by the plain source only, so host rays
    never get there."""
    if scene == "ripple":
        pts, nrm, gd = _rippled_surface()
        D = 3
    else:
        _, D, gd, pts, nrm = er.geometry(scene)
    shift = np.array([2048, -1024, 512 if D == 3 else 0], dtype=np.float32)
    far = (pts.astype(np.float32) + shift).astype(np.float32)
    rays = 500 if D == 2 else 20
    bcs = er.boundary_conditions(D)

    def tracer(p):
        t = vr.TraceDisk(D)
        t.setGeometry(p, nrm, gd)
        t.setBoundaryConditions(bcs)
        if D == 2:
            t.setSourceDirection(TD.POS_Y)
        t.setParticleType(vr.DiffuseParticle(sticking, "flux"))
        t.setNumberOfRaysPerPoint(rays)
        t.setRngSeed(77)
        return t

    near = tracer(pts)
    near.apply()
    t = tracer(far)
    t.apply()
    assert t.traceMode() == near.traceMode() == FAR_MODES[scene][sticking], (t.traceMode(), near.traceMode())
    orc = po.Oracle()
    orc.set_disks(far, nrm, gd, D)
    orc.set_boundary_conditions([int(b) for b in bcs])
    if D == 2:
        orc.set_source_direction(po.POS_Y)
    orc.set_particle(po.DIFFUSE, sticking)
    orc.set_num_rays_per_point(rays)
    orc.set_rng_seed(77)
    orc.set_lazy_rng(True)
    orc.apply(po.max_threads())
    oi = orc.info()
    gi = info_dict(t)
    f, r = np.asarray(t.getLocalData().getVectorData(0)), orc.flux()
    print(scene, sticking, gi, "l2_rel", l2_rel(f, r))
    assert gi == {k: oi[k] for k in INFO_KEYS}
    assert gi["geometryHits"] > 0 and gi["boundaryHits"] > 0
    if sticking >= 1.0:
        assert (f == r).all(), l2_rel(f, r)
    assert l2_rel(f, r) <= 5e-6
    assert l2_rel(t.normalizeFlux(f), orc.normalize_flux(r)) <= 1e-4
    a, b = t.getDiskAreas(), orc.disk_areas()
    assert (np.isnan(a) == np.isnan(b)).all()
    ok = ~np.isnan(b)
    assert np.allclose(a[ok], b[ok], rtol=1e-5, atol=1e-6)
