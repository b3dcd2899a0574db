"""The planar kernel's one-point-per-round form (VR_PLANAR_ROUND; trace_kernel MODE_ABSORB_FLAT_PLANAR_ROUND, pq_hit_packet
ROUND, vr_planar_disks.hpp (1) - (3)): the plane hit of a ray serves both candidate tests, the query's box is the box around
the wave's hit points, and a round whose rays all start inside the walls and land well inside them runs no wall test
but for the lanes the query left without a hit.  That only removes work: every scene runs once with VR_PLANAR_ROUND=0 (the
planar kernel as it was) and once with =1, and the raw float32 and float64 flux arrays are equal element for element, as
is every TraceInfo counter; each run also goes against the CPU oracle with the bounds of tests/test_planar_disks.py
(counters equal, flux L2-relative error <= 5e-6, <= 1e-4 on the source-normalised flux).  The VR_PRINT_LAUNCHES lines say
which kernel the launch ran.

The scenes: disks on a 32 x 32 lattice of pitch 1, 200 000 rays, seed 12345, DiffuseParticle of sticking 1 — on a domain
this small most rounds have a lane near a wall, so both the wall-free rounds and the others run.  (a) periodic walls;
(b) reflective walls; (c) periodic along x, reflective along y; (d) a 6 x 6 block of disks removed: misses in rounds that
are wall-free otherwise, which the wall test behind the query still has to see; (e1) / (e2) normals (0, 0, -1) under POS_Z
(every disk met from behind, nothing credited) and under NEG_Z; (f) the plane x = 0.3f under POS_X; (g) a 64 x 64 lattice
under 4 000 000 rays: full waves, wall-free interior rounds, several leaf nodes per query; (h) one centre an ulp off the
plane: not planar, neither planar kernel runs."""
import functools
import re

import numpy as np
import pytest

import viennaray_amd as vr
from viennaray_amd import BoundaryCondition as BC
from oracle import pyoracle as po
from helpers import l2_rel

pytestmark = pytest.mark.gpu

COUNTERS = ("numRays", "totalRaysTraced", "nonGeometryHits", "geometryHits", "particleHits", "boundaryHits", "reflections",
            "raysTerminated", "rngFullStates")
ORACLE_COUNTERS = ("totalRaysTraced", "nonGeometryHits", "geometryHits", "boundaryHits", "reflections", "raysTerminated")
FLUX_ORDER_TOL = 5e-6  # tests/test_planar_disks.py: identical rays, only the float summation order differs
FLUX_TOL = 1e-4        # ... and on the source-normalised flux
SEED = 12345
P, R = BC.PERIODIC_BOUNDARY, BC.REFLECTIVE_BOUNDARY
ORACLE_BC = {P: po.PERIODIC, R: po.REFLECTIVE}


@functools.lru_cache(maxsize=None)
def scene(name):
    """points, normals (read-only arrays), the number of rays, the source direction and the boundary conditions"""
    n, rays = (64, 4_000_000) if name == "g" else (32, 200_000)
    x0 = -(n - 1) / 2.0
    X, Y = np.meshgrid(x0 + np.arange(n), x0 + np.arange(n), indexing="ij")
    height = np.float32(0.3) if name in ("f", "h") else np.float32(0.0)
    pts = np.stack([X.ravel(), Y.ravel(), np.full(n * n, height)], -1).astype(np.float32)
    nrm = np.tile(np.array([0, 0, 1], np.float32), (n * n, 1))
    direction = vr.TraceDirection.POS_Z
    bcs = {"b": (R, R, R), "c": (P, R, P)}.get(name, (P, P, P))
    if name == "d":  # a hole in the middle of the lattice
        i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
        keep = ~((i >= 13) & (i < 19) & (j >= 13) & (j < 19)).ravel()
        assert keep.sum() == n * n - 36
        pts, nrm = pts[keep], nrm[keep]
    if name in ("e1", "e2"):
        nrm = np.tile(np.array([0, 0, -1], np.float32), (len(pts), 1))
    if name == "e2":
        direction = vr.TraceDirection.NEG_Z
    if name == "f":
        pts = np.ascontiguousarray(pts[:, [2, 0, 1]])  # the plane x = 0.3f
        nrm = np.tile(np.array([1, 0, 0], np.float32), (len(pts), 1))
        direction = vr.TraceDirection.POS_X
    if name == "h":
        k = 13 * n + 17  # an interior disk
        pts[k, 2] = np.nextafter(pts[k, 2], np.float32(1))
        assert int(pts[k, 2].view(np.uint32)) == int(height.view(np.uint32)) + 1
    pts = np.ascontiguousarray(pts)
    nrm = np.ascontiguousarray(nrm)
    pts.setflags(write=False)
    nrm.setflags(write=False)
    return pts, nrm, rays, direction, bcs


def gpu_run(name, knob, monkeypatch, capfd):
    monkeypatch.setenv("VR_SMALL_SCENE", "0")
    monkeypatch.setenv("VR_PLANAR_ROUND", str(knob))
    monkeypatch.setenv("VR_PRINT_LAUNCHES", "1")
    pts, nrm, rays, direction, bcs = scene(name)
    t = vr.TraceDisk(3)
    t.setGeometry(pts, nrm, 1.0)
    t.setBoundaryConditions(list(bcs))
    t.setSourceDirection(direction)
    t.setParticleType(vr.DiffuseParticle(1.0, "flux"))
    t.setNumberOfRaysFixed(rays)
    t.setRngSeed(SEED)
    capfd.readouterr()
    t.apply()
    err = capfd.readouterr().err
    pla = re.search(r"\[vr\] planar disks: scene (\d), VR_PLANAR_DISKS (\d), launch (\d)", err)
    rnd = re.search(r"\[vr\] planar disks: round: VR_PLANAR_ROUND (\d), launch (\d)", err)
    assert pla, "no planar-disks line on stderr"
    assert rnd, "no planar-round line on stderr"
    assert err.index("[vr] planar disks: scene") < err.index("[vr] planar disks: round:")
    info = t.getRayTraceInfo()
    return {"t": t, "f32": t.getLocalData().getVectorData(0).copy(), "f64": t.getFluxF64(), "mode": t.traceMode(),
            "info": {k: int(getattr(info, k)) for k in COUNTERS}, "planar": tuple(int(v) for v in pla.groups()),
            "round": tuple(int(v) for v in rnd.groups())}


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    pts, nrm, rays, direction, bcs = scene(name)
    o = po.Oracle()
    o.set_disks(pts, nrm, 1.0, 3)
    o.set_boundary_conditions([ORACLE_BC[b] for b in bcs])
    o.set_source_direction(int(direction))
    o.set_particle(po.DIFFUSE, 1.0)
    o.set_num_rays_fixed(rays)
    o.set_rng_seed(SEED)
    o.set_lazy_rng(True)
    o.apply(po.max_threads())
    return o, o.flux(), o.info()


def against_oracle(name, run):
    o, ref, oi = oracle_run(name)
    assert {k: run["info"][k] for k in ORACLE_COUNTERS} == {k: oi[k] for k in ORACLE_COUNTERS}, (run["info"], oi)
    if not ref.any():  # (e1: nothing is credited, by the oracle either)
        assert not run["f32"].any()
        return
    err = l2_rel(run["f32"], ref)
    print("  oracle L2", err, {k: oi[k] for k in ORACLE_COUNTERS})
    assert err <= FLUX_ORDER_TOL, err
    assert l2_rel(run["t"].normalizeFlux(run["f32"]), o.normalize_flux(ref)) <= FLUX_TOL


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e1", "e2", "f", "g"])
def test_round_form_changes_no_result(name, monkeypatch, capfd):
    off = gpu_run(name, 0, monkeypatch, capfd)
    on = gpu_run(name, 1, monkeypatch, capfd)
    print(name, "modes", off["mode"], on["mode"], "planar", off["planar"], on["planar"], "round", off["round"], on["round"], on["info"])
    assert off["mode"] == 1 and on["mode"] == 1  # (the flat absorbing kernel; the form is a kernel of that mode)
    assert off["planar"] == (1, 1, 1) and on["planar"] == (1, 1, 1)  # a planar kernel ran both times
    assert off["round"] == (0, 0)  # the knob forces the launch's flag false: the planar kernel as it was
    assert on["round"] == (1, 1)
    assert on["info"] == off["info"], (off["info"], on["info"])
    i = on["info"]
    if name == "e1":  # (the disks face away from the source: met from behind, the ray goes on; nothing is credited)
        assert i["geometryHits"] == 0 and i["totalRaysTraced"] - i["numRays"] - i["boundaryHits"] > 0, i
        assert on["f64"].sum() == 0 and off["f64"].sum() == 0
    else:
        assert i["geometryHits"] > 0
        assert on["f64"].sum() > 0
    if name == "d":
        assert i["nonGeometryHits"] > 0, i  # rays through the hole
    if name in ("b", "c"):
        assert i["boundaryHits"] > 0, i
    assert np.array_equal(off["f64"], on["f64"])
    assert np.array_equal(off["f32"], on["f32"])
    against_oracle(name, off)
    against_oracle(name, on)


def test_one_centre_an_ulp_off_the_plane_runs_neither_planar_kernel(monkeypatch, capfd):
    run = gpu_run("h", 1, monkeypatch, capfd)
    print("h: planar", run["planar"], "round", run["round"], run["info"])
    assert run["mode"] == 1
    assert run["planar"] == (0, 1, 0)
    assert run["round"] == (1, 0)  # the knob is on, the launch does not take the form
    assert run["info"]["geometryHits"] > 0
    against_oracle("h", run)
