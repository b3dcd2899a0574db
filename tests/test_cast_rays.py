"""Closest-hit queries for the caller's rays on the device (vr_cast_rays, vr_cast_rays_device; Trace.castRays /
occluded) against the oracle: one segment against its brute force on every edge-case family of tests/edge_rays.py, and
followed chains against a chain built in Python from the oracle's brute force and its Boundary::processHit.  Everything
is compared bit for bit — primitive, float32 path length, boundary hits, end point: both sides run the same float
operations in the same order (-ffp-contract=off).  Then the launch's shape (grid-stride loop, stack slabs, the ray sort),
tails, tmax, tensors and streams, refusals, and what a cast must leave alone: a finished apply's flux and the next apply."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import viennaray_amd as vr
from viennaray_amd import capi
import edge_rays as er

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISS, WALL = capi.VR_CAST_MISS, capi.VR_CAST_WALL
BC = vr.BoundaryCondition
NEVER = "4294967295"
INF = np.float32(np.inf)
TNEAR = 1e-4
BUDGET = 3  # maxBoundaryHits of the chains: some rays stop on a wall, some pass a wall or two and land (checked below)
CHAIN_RAYS = 256
CHAIN_FAMILIES = ("axis", "graze", "wall_edge")
# (scene, boundary conditions by axis; None: er.boundary_conditions(D))
CHAIN_CELLS = (("trench3d", None), ("trench2d", None), ("mesh", None),
               ("trench3d", (BC.PERIODIC_BOUNDARY, BC.IGNORE_BOUNDARY, BC.REFLECTIVE_BOUNDARY)))


def _torch():
    import torch
    return torch


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _bcs(scene, bcs):
    return list(bcs) if bcs is not None else er.boundary_conditions(er.scene(scene).D)


@functools.lru_cache(maxsize=None)
def _tracer(scene, bcs=None):
    """one tracer per scene and boundary conditions with one prepare behind it: what a cast reads is resident"""
    t = er.new_tracer(scene)
    if bcs is not None:
        t.setBoundaryConditions(list(bcs))
    t.setParticleType(vr.DiffuseParticle(1.0, "f"))
    t.setNumberOfRaysFixed(1000)
    t.applyPrepare()
    return t


# ---------------------------------------------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------------------------------------------
def expected_one_segment(ref):
    """(prim, dist) of a cast that follows no wall, from the oracle's (geomID, primID, t)"""
    g, p, t = ref
    prim = np.where(g == 1, p.astype(np.int64), np.where(g == 0, WALL, MISS)).astype(np.int32)
    dist = np.where(g >= 0, t, INF).astype(np.float32)
    return prim, dist


@functools.lru_cache(maxsize=None)
def _chain_oracle(scene, bcs):
    orc = er.new_oracle(scene)
    orc.set_boundary_conditions([int(b) for b in _bcs(scene, bcs)])
    orc.prepare()
    return orc


def chain_one(orc, o, d, budget, follow=True):
    """One ray the way the definition has it, from the oracle alone: brute-force closest hit, Boundary::processHit at a
    wall, float32 distances added in segment order.  (prim, dist, boundaryHits, end point)"""
    nan3 = np.full(3, np.nan, dtype=np.float32)
    org, dr, rd = o.astype(np.float32), d.astype(np.float32), d.astype(np.float32)
    dist, hits = np.float32(0), 0
    while True:
        h = orc.intersect1(org, dr, TNEAR, brute=True)
        if h["geomID"] < 0:
            return MISS, INF, hits, nan3
        t = np.float32(h["t"])
        dist = np.float32(dist + t)
        point = (org + dr * t).astype(np.float32)  # (float32 product, then float32 sum: the tracer's expression)
        if h["geomID"] == 1:
            return int(h["primID"]), dist, hits, point
        if not follow or hits + 1 > budget:
            return WALL, dist, hits, point
        r = orc.boundary_process_hit(org, dr, float(t), int(h["primID"]), ray_direction=rd)
        if not r["reflect"]:  # an IGNORE wall: the ray leaves
            return MISS, INF, hits, nan3
        hits += 1
        org, dr, rd = r["org"], r["dir"], r["rayDirection"]


def chain_rays(scene):
    fams = er.scene_families(scene)
    o = np.concatenate([fams[f][0][:CHAIN_RAYS] for f in CHAIN_FAMILIES])
    d = np.concatenate([fams[f][1][:CHAIN_RAYS] for f in CHAIN_FAMILIES])
    return o, d


@functools.lru_cache(maxsize=None)
def chain_reference(scene, bcs, budget=BUDGET):
    """(prim i32, dist f32, boundaryHits i32, points f32[m, 3]) of the CHAIN_FAMILIES' first CHAIN_RAYS rays each"""
    orc = _chain_oracle(scene, bcs)
    o, d = chain_rays(scene)
    rows = [chain_one(orc, o[i], d[i], budget) for i in range(len(o))]
    out = (np.array([r[0] for r in rows], np.int32), np.array([r[1] for r in rows], np.float32),
           np.array([r[2] for r in rows], np.int32), np.stack([r[3] for r in rows]).astype(np.float32))
    for a in out:
        a.setflags(write=False)
    return out


def _same_point_bits(a, b):
    """rows equal bit for bit, a NaN row equal to a NaN row"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (_bits(a) == _bits(b)).all(axis=1) | (np.isnan(a).all(axis=1) & np.isnan(b).all(axis=1))


def _first_difference(o, d, got, want, what):
    prim, dist, hits, pts = got
    prim0, dist0, hits0, pts0 = want
    bad = (prim != prim0) | (_bits(dist) != _bits(dist0))
    if hits is not None:
        bad |= hits != hits0
    if pts is not None:
        bad |= ~_same_point_bits(pts, pts0)
    bad = np.flatnonzero(bad)
    if bad.size:
        i = bad[0]
        pytest.fail("%s: %d of %d rays differ; first is ray %d: %s\n  expected: prim %d dist %s hits %s point %s\n  device:   "
                    "prim %d dist %s hits %s point %s" % (
                        what, bad.size, len(prim), i, er.hexray(o[i], d[i]), prim0[i], float(dist0[i]).hex(),
                        None if hits is None else hits0[i], None if pts is None else [float(x).hex() for x in pts0[i]],
                        prim[i], float(dist[i]).hex(), None if hits is None else hits[i],
                        None if pts is None else [float(x).hex() for x in pts[i]]))


# ---------------------------------------------------------------------------------------------------------------
# 1. one segment equals the oracle's brute force
# ---------------------------------------------------------------------------------------------------------------
SEGMENT_CELLS = [(s, f) for s in er.SCENES for f in er.family_names(s)]
SEGMENT_CELLS += [(er.KNOWN_ANSWERS[k][0], k) for k in sorted(er.KNOWN_ANSWERS)]


@pytest.mark.parametrize("scene,family", SEGMENT_CELLS, ids=["%s-%s" % c for c in SEGMENT_CELLS])
def test_one_segment_equals_brute_force(scene, family):
    """following off, the tracer's tnear: every ray of every family — a primitive with the bits of t, VR_CAST_WALL with the
    bits of t, or (-1, +inf)"""
    if family in er.KNOWN_ANSWERS:
        o, d, ref = er.known_answer(family)
    else:
        o, d = er.scene_families(scene)[family]
        ref = er.reference(scene, family)
    prim, dist, hits = _tracer(scene).castRays(o, d, followBoundaries=False, tnear=TNEAR, returnBoundaryHits=True)
    assert prim.dtype == np.int32 and dist.dtype == np.float32 and prim.shape == dist.shape == (len(o),)
    want = expected_one_segment(ref)
    _first_difference(o, d, (prim, dist, hits, None), want + (np.zeros(len(o), np.int32), None), "%s/%s" % (scene, family))


# ---------------------------------------------------------------------------------------------------------------
# 2. followed chains equal a chain built from the oracle
# ---------------------------------------------------------------------------------------------------------------
def _cast_chain(scene, bcs, o, d, budget=BUDGET, **kw):
    t = _tracer(scene, bcs if bcs is not None else tuple(_bcs(scene, None)))
    t.setMaxBoundaryHits(budget)
    return t.castRays(o, d, returnPoints=True, returnBoundaryHits=True, **kw)


def _reorder(out):
    prim, dist, pts, hits = out
    return prim, dist, hits, pts


@pytest.mark.parametrize("scene,bcs", CHAIN_CELLS, ids=["%s-%s" % (s, "default" if b is None else "mixed") for s, b in CHAIN_CELLS])
def test_followed_chains_equal_the_oracle(scene, bcs):
    o, d = chain_rays(scene)
    want = chain_reference(scene, bcs)
    got = _reorder(_cast_chain(scene, bcs, o, d))
    _first_difference(o, d, got, want, "%s chains" % scene)
    assert got[2].dtype == np.int32 and got[3].shape == (len(o), 3)
    print(scene, "walls", int((want[0] == WALL).sum()), "misses", int((want[0] == MISS).sum()),
          "landed behind a wall", int(((want[0] >= 0) & (want[2] >= 1)).sum()))


def test_the_chains_reach_the_budget_and_land_behind_walls():
    """what the budget of 3 was chosen for, on the oracle's answers alone: rays that stop on a wall, rays that pass at
    least one wall and still hit geometry, and (the mixed conditions) rays that leave through an IGNORE wall"""
    stopped = landed = 0
    for scene, bcs in CHAIN_CELLS:
        prim, _, hits, _ = chain_reference(scene, bcs)
        stopped += int((prim == WALL).sum())
        landed += int(((prim >= 0) & (hits >= 1)).sum())
        assert ((prim == WALL) <= (hits == BUDGET)).all()  # (a followed ray only ever stops on a wall with the budget spent)
    assert stopped >= 1 and landed >= 1, (stopped, landed)
    prim, _, hits, _ = chain_reference(*CHAIN_CELLS[3])
    assert int((prim == MISS).sum()) > int((chain_reference(*CHAIN_CELLS[0])[0] == MISS).sum())


# ---------------------------------------------------------------------------------------------------------------
# 3. grid-stride loop, slabs and permutation
# ---------------------------------------------------------------------------------------------------------------
def test_many_rays_sorted_unsorted_and_in_chunks_give_the_same_bits(monkeypatch):
    """600 001 rays: more groups of 64 than the launch may have waves (at most 32 per CU), and a last group of one ray —
    every wave takes several groups and keeps its slab.  Sorted by origin, unsorted, and in casts of 1500: identical."""
    o0, d0 = chain_rays("trench3d")
    m = 600_001
    rep = -(-m // len(o0))
    o, d = np.tile(o0, (rep, 1))[:m], np.tile(d0, (rep, 1))[:m]
    monkeypatch.setenv("VR_CAST_SORT_MIN", "0")
    a = _cast_chain("trench3d", None, o, d)
    monkeypatch.setenv("VR_CAST_SORT_MIN", NEVER)
    b = _cast_chain("trench3d", None, o, d)
    chunks = [_cast_chain("trench3d", None, o[k:k + 1500], d[k:k + 1500]) for k in range(0, m, 1500)]
    c = tuple(np.concatenate([ch[j] for ch in chunks]) for j in range(4))
    for other, what in ((b, "unsorted"), (c, "chunks")):
        assert np.array_equal(a[0], other[0]), what
        assert np.array_equal(_bits(a[1]), _bits(other[1])), what
        assert _same_point_bits(a[2], other[2]).all(), what
        assert np.array_equal(a[3], other[3]), what
    # ... and they are the oracle's, tiled
    want = chain_reference("trench3d", None)
    n0 = len(o0)
    _first_difference(o[-n0:], d[-n0:], tuple(x[m - n0:] for x in _reorder(a)),
                      tuple(np.roll(w, -((m - n0) % n0), axis=0) for w in want), "the last rows of the large cast")


# ---------------------------------------------------------------------------------------------------------------
# 4. tails
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sort", ("0", NEVER), ids=("sorted", "unsorted"))
def test_tails(sort, monkeypatch):
    monkeypatch.setenv("VR_CAST_SORT_MIN", sort)
    o, d = chain_rays("mesh")
    full = _cast_chain("mesh", None, o, d)
    for m in (1, 63, 64, 65):
        part = _cast_chain("mesh", None, o[:m], d[:m])
        assert all(x.shape[0] == m for x in part)
        assert np.array_equal(part[0], full[0][:m]) and np.array_equal(_bits(part[1]), _bits(full[1][:m])), m
        assert _same_point_bits(part[2], full[2][:m]).all() and np.array_equal(part[3], full[3][:m]), m
    empty = _cast_chain("mesh", None, np.empty((0, 3), np.float32), np.empty((0, 3), np.float32))
    assert [x.shape for x in empty] == [(0,), (0,), (0, 3), (0,)]
    assert [x.dtype for x in empty] == [np.int32, np.float32, np.float32, np.int32]


# ---------------------------------------------------------------------------------------------------------------
# 5. tmax
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ("trench3d", "trench2d"))
def test_tmax_turns_what_lies_beyond_into_a_miss(scene):
    o, d = chain_rays(scene)
    prim, dist, pts, hits = _cast_chain(scene, None, o, d)
    finite = dist[np.isfinite(dist)]
    tmax = np.float32(np.median(finite))
    beyond = dist > tmax  # (misses included: +inf)
    assert 0 < int((~beyond).sum()) and int((beyond & (prim != MISS)).sum()) > 0
    got = _cast_chain(scene, None, o, d, tmax=float(tmax))
    assert np.array_equal(got[0], np.where(beyond, MISS, prim))
    assert np.array_equal(_bits(got[1]), _bits(np.where(beyond, INF, dist)))
    assert np.isnan(got[2][beyond]).all() and _same_point_bits(got[2][~beyond], pts[~beyond]).all()
    assert np.array_equal(got[3], np.where(beyond, 0, hits))  # (a miss under a finite tmax reports no walls)
    # tmax = 0 misses everything
    zero = _cast_chain(scene, None, o, d, tmax=0.0)
    assert (zero[0] == MISS).all() and np.isinf(zero[1]).all() and np.isnan(zero[2]).all() and (zero[3] == 0).all()
    # a hit at exactly tmax counts: the ray behind a wall with the longest path that landed
    landed = np.flatnonzero((prim >= 0) & (hits >= 1))
    k = int(landed[np.argmax(dist[landed])]) if landed.size else int(np.flatnonzero(prim >= 0)[0])
    exact = _cast_chain(scene, None, o[k:k + 1], d[k:k + 1], tmax=float(dist[k]))
    assert exact[0][0] == prim[k] and _bits(exact[1])[0] == _bits(dist)[k] and exact[3][0] == hits[k]
    below = _cast_chain(scene, None, o[k:k + 1], d[k:k + 1], tmax=float(np.nextafter(dist[k], np.float32(0))))
    assert below[0][0] == MISS and np.isinf(below[1][0])


# ---------------------------------------------------------------------------------------------------------------
# 6. tensors, streams, refusals
# ---------------------------------------------------------------------------------------------------------------
def test_tensors_on_another_stream_equal_the_host_form():
    torch = _torch()
    o, d = chain_rays("trench3d")
    want = _cast_chain("trench3d", None, o, d)
    t = _tracer("trench3d", tuple(_bcs("trench3d", None)))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        do, dd = _dev(o), _dev(d)
        got = t.castRays(do, dd, returnPoints=True, returnBoundaryHits=True)
        two = t.castRays(do, dd)
    s.synchronize()
    assert all(x.is_cuda for x in got) and len(two) == 2
    assert [x.dtype for x in got] == [torch.int32, torch.float32, torch.float32, torch.int32]
    got = [x.cpu().numpy() for x in got]
    assert np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1]))
    assert _same_point_bits(got[2], want[2]).all() and np.array_equal(got[3], want[3])
    assert np.array_equal(two[0].cpu().numpy(), want[0])


def test_rows_of_two_floats_on_a_two_dimensional_tracer():
    o, d = chain_rays("trench2d")
    assert not o[:, 2].any() and not d[:, 2].any()
    want = _cast_chain("trench2d", None, o, d)
    host2 = _cast_chain("trench2d", None, o[:, :2], d[:, :2])
    t = _tracer("trench2d", tuple(_bcs("trench2d", None)))
    dev2 = [x.cpu().numpy() for x in t.castRays(_dev(o[:, :2]), _dev(d[:, :2]), returnPoints=True, returnBoundaryHits=True)]
    for got in (host2, dev2):
        assert np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1]))
        assert _same_point_bits(got[2], want[2]).all() and np.array_equal(got[3], want[3])
    with pytest.raises(ValueError):  # two columns need a 2-D tracer
        _tracer("trench3d", tuple(_bcs("trench3d", None))).castRays(_dev(o[:, :2]), _dev(d[:, :2]))


def _call(t, o, d, m, ld, tnear, tmax, flags, prim, dist, pts=None, hits=None):
    ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data)
    rc = t._L.vr_cast_rays_device(t._h, ptr(o), ptr(d), m, ld, tnear, tmax, flags, ptr(prim), ptr(dist), ptr(pts), ptr(hits), None)
    return rc, t._L.vr_last_error(t._h).decode()


def test_refusals_leave_the_outputs_untouched_and_the_context_usable():
    torch = _torch()
    o, d = chain_rays("trench3d")
    m = len(o)
    t = _tracer("trench3d", tuple(_bcs("trench3d", None)))
    do, dd = _dev(o), _dev(d)
    prim = torch.full((m,), -7, dtype=torch.int32, device="cuda")
    dist = torch.full((m,), -7.0, dtype=torch.float32, device="cuda")
    pts = torch.full((m, 3), -7.0, dtype=torch.float32, device="cuda")
    hits = torch.full((m,), -7, dtype=torch.int32, device="cuda")
    inf, follow = float("inf"), capi.VR_CAST_FOLLOW_BOUNDARIES

    def refused(word, *args):
        rc, msg = _call(t, *args)
        torch.cuda.synchronize()
        assert rc == capi.VR_E_INVALID and "vr_cast_rays_device" in msg and word in msg, (rc, msg)
        assert bool((prim == -7).all()) and bool((dist == -7.0).all()) and bool((pts == -7.0).all()) and bool((hits == -7).all())

    refused("device memory", o, dd, m, 3, TNEAR, inf, follow, prim, dist, pts, hits)  # a host pointer as origins
    refused("device memory", do, dd, m, 3, TNEAR, inf, follow, prim, dist, np.empty((m, 3), np.float32), hits)
    refused("ld is 2 or 3", do, dd, m, 4, TNEAR, inf, follow, prim, dist, pts, hits)
    refused("2-D scene", do, dd, m, 2, TNEAR, inf, follow, prim, dist, pts, hits)
    refused("tmax", do, dd, m, 3, TNEAR, -1.0, follow, prim, dist, pts, hits)
    refused("tmax", do, dd, m, 3, TNEAR, float("nan"), follow, prim, dist, pts, hits)
    refused("tnear", do, dd, m, 3, -1e-4, inf, follow, prim, dist, pts, hits)
    refused("flag", do, dd, m, 3, TNEAR, inf, 2, prim, dist, pts, hits)
    refused("null", do, None, m, 3, TNEAR, inf, follow, prim, dist, pts, hits)
    refused("null", do, dd, m, 3, TNEAR, inf, follow, None, dist, pts, hits)
    rc, _ = _call(t, do, dd, 0, 3, TNEAR, inf, follow, prim, dist, pts, hits)  # m == 0: fine, nothing touched
    torch.cuda.synchronize()
    assert rc == capi.VR_OK and bool((prim == -7).all())
    t.setMaxBoundaryHits(BUDGET)
    rc, msg = _call(t, do, dd, m, 3, TNEAR, inf, follow, prim, dist, pts, hits)  # and a valid call works
    torch.cuda.synchronize()
    assert rc == capi.VR_OK, msg
    assert np.array_equal(prim.cpu().numpy(), chain_reference("trench3d", None)[0])
    # tensors that cannot go as they are
    for bad in (do.double(), do.cpu(), do.t().contiguous().t()):
        with pytest.raises(ValueError):
            t.castRays(bad, dd)
        with pytest.raises(ValueError):
            t.castRays(do, bad)
    with pytest.raises(ValueError):
        t.castRays(do, dd[:-1])
    with pytest.raises(ValueError):
        t.castRays(o, dd)  # a host array beside a tensor
    with pytest.raises(vr.VrError):
        t.castRays(o, d, tmax=-1.0)  # the host form refuses as well
    assert t.castRays(do, dd)[0].shape == (m,)


# ---------------------------------------------------------------------------------------------------------------
# 7. state
# ---------------------------------------------------------------------------------------------------------------
def _info(t):
    i = t.getRayTraceInfo()
    return {k: int(getattr(i, k)) for k in ("numRays", "totalRaysTraced", "nonGeometryHits", "geometryHits", "particleHits",
                                            "boundaryHits", "reflections", "raysTerminated")}


def _state_tracer(sticking=0.3):
    t = er.new_tracer("trench3d")
    t.setBoundaryConditions(er.boundary_conditions(3))
    t.setParticleType(vr.DiffuseParticle(sticking, "flux"))
    t.setNumberOfRaysFixed(50_000)
    t.setUseRandomSeeds(False)
    t.setRngSeed(4711)
    t.setMaxBoundaryHits(BUDGET)
    return t


def test_a_cast_needs_what_a_prepare_left_for_the_settings_in_force():
    o, d = chain_rays("trench3d")
    want = chain_reference("trench3d", None)
    t = _state_tracer()

    def refused():
        with pytest.raises(vr.VrError, match="nothing to cast against"):
            t.castRays(o, d)
        m = len(o)
        prim, dist = np.full(m, -7, np.int32), np.full(m, -7, np.float32)
        rc = t._L.vr_cast_rays(t._h, o.ctypes.data_as(C.POINTER(C.c_float)), d.ctypes.data_as(C.POINTER(C.c_float)), m, TNEAR,
                               float("inf"), 1, prim.ctypes.data_as(C.POINTER(C.c_int32)),
                               dist.ctypes.data_as(C.POINTER(C.c_float)), None, None)
        assert rc == capi.VR_E_STATE and (prim == -7).all() and (dist == -7).all()

    def works():
        got = _reorder(t.castRays(o, d, returnPoints=True, returnBoundaryHits=True))
        _first_difference(o, d, got, want, "after apply")

    refused()  # before any prepare
    t.apply()
    works()
    kind, D, gd, pts, nrm = er.geometry("trench3d")
    t.setGeometry(pts[:-7], nrm[:-7], gd)  # another geometry
    refused()
    t.setGeometry(pts, nrm, gd)
    refused()  # (set anew: the resident build is the previous geometry's)
    t.apply()
    works()
    t.setBoundaryConditions([BC.PERIODIC_BOUNDARY, BC.IGNORE_BOUNDARY, BC.REFLECTIVE_BOUNDARY])  # other conditions
    refused()
    t.setBoundaryConditions(er.boundary_conditions(3))
    t.apply()
    works()
    t.setSourceDirection(vr.TraceDirection.NEG_Z)  # the walls and the child order follow it
    refused()
    t.setSourceDirection(vr.TraceDirection.POS_Z)
    t.applyPrepare()  # a prepare is enough
    works()


def test_a_cast_leaves_the_flux_and_the_next_apply_alone():
    o, d = chain_rays("trench3d")
    a = _state_tracer()
    a.apply()
    f0, i0 = a.getFluxF64().copy(), _info(a)
    t0 = a.getFluxTensor().cpu().numpy()
    a.castRays(o, d)
    a.castRays(_dev(o), _dev(d), returnPoints=True)
    assert np.array_equal(a.getFluxF64(), f0) and np.array_equal(_bits(a.getFluxTensor().cpu().numpy()), _bits(t0))
    assert f0.sum() > 0
    a.apply()
    b = _state_tracer()
    b.apply()
    assert np.array_equal(b.getFluxF64(), f0) and _info(b) == i0  # (the same first apply)
    b.apply()
    assert np.array_equal(a.getFluxF64(), b.getFluxF64()) and _info(a) == _info(b)
    assert a.traceMode() == b.traceMode()


# ---------------------------------------------------------------------------------------------------------------
# 8. occluded
# ---------------------------------------------------------------------------------------------------------------
def test_occluded_on_a_plane():
    s = er.scene("plane")
    rng = np.random.default_rng(8)
    m = 300
    o = rng.uniform(s.lo * 0.8, s.hi * 0.8, (m, 3)).astype(np.float32)
    o[:, 2] = rng.uniform(0.5, 3.0, m).astype(np.float32)
    below = rng.uniform(s.lo * 0.8, s.hi * 0.8, (m, 3)).astype(np.float32)
    below[:, 2] = -rng.uniform(0.5, 3.0, m).astype(np.float32)
    beside = o + rng.uniform(-2.0, 2.0, (m, 3)).astype(np.float32) * np.array([1, 1, 0], np.float32)
    above = o.copy()
    above[:, 2] += 5
    t = _tracer("plane")
    assert t.occluded(o, below).all() and t.occluded(o, below).dtype == bool
    assert not t.occluded(o, beside).any() and not t.occluded(o, above).any()
    # the segment ends at the target: a target above the plane on the way down is not occluded, the same ray longer is
    short = o.copy()
    short[:, 2] = 0.25
    assert not t.occluded(o, short).any() and t.occluded(o, 2 * below - o).all()
    dev = t.occluded(_dev(o), _dev(below))
    assert dev.is_cuda and bool(dev.all()) and not bool(t.occluded(_dev(o), _dev(beside)).any())


# ---------------------------------------------------------------------------------------------------------------
# the C++ façade
# ---------------------------------------------------------------------------------------------------------------
FACADE_FLAGS = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include",
                "-I", os.path.join(ROOT, "include", "viennaray_amd"), "-I", os.path.join(ROOT, "include")]


def test_cpp_facade_cast_rays(tmp_path):
    """tests/aux/facade_cast_rays.cpp: castRays on a sheet of disks — the centre disk for a vertical ray at its centre, a
    miss for a ray pointing up — and castRaysDevice word for word the host form"""
    src = os.path.join(ROOT, "tests", "aux", "facade_cast_rays.cpp")
    exe = tmp_path / "facade_cast_rays"
    lib = os.path.join(ROOT, "viennaray_amd")
    subprocess.check_call(["g++", "-O1"] + FACADE_FLAGS + [src, "-o", str(exe), "-L", lib, "-lviennaray_amd",
                                                          "-L", "/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib,
                                                          "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "facade cast rays ok" in out.stdout, out.stdout + out.stderr
