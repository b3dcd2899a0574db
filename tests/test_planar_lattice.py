"""The one-point-per-round kernel with its candidates from the lattice table (VR_PLANAR_LATTICE; MODE_ABSORB_FLAT_LATTICE,
pq_hit_lattice, vr_planar_lattice.hpp): where the centres of a planar cloud sit on a square
lattice of pitch gridDelta, the disks near a round's box are the lattice points of an index window, and the parent's
ball-box filter on their records leaves the parent's candidates.  That only removes the search: every scene runs once with
VR_PLANAR_LATTICE=0 (the one-point-per-round kernel as it was) and once with =1, and the raw float32 and float64 flux
arrays are equal element for element, as is every TraceInfo counter; each run also goes against the CPU oracle with the
bounds of tests/test_planar_round.py (counters equal, flux L2-relative error <= 5e-6, <= 1e-4 on the source-normalised
flux).  The VR_PRINT_LAUNCHES lines say which kernel the launch ran.

The scenes, DiffuseParticle of sticking 1, seed 12345: (a) / (b) / (c) of tests/test_planar_round.py — a 32 x 32 lattice of
pitch 1 under 200 000 rays with periodic, reflective and mixed walls: most rounds touch a wall and the window is clamped
at the table's edge; (d) a 6 x 6 block of disks removed: empty cells and misses; (f) the plane x = 0.3f under POS_X;
(g) a 64 x 64 lattice under 4 000 000 rays: full waves; (r) a 32 x 48 lattice: a row / column swap would show; (p) pitch
0.5 with gridDelta 0.5; (s) the lattice's phase at 0.37: nothing is symmetric about 0; (j) every centre jittered by up to
0.05 gridDelta in the plane, seeded: still a lattice cloud.  Not lattice clouds, the launch keeps the parent's kernel:
(m) one centre moved by 0.3 gridDelta in the plane; (u) one centre twice."""
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
FLUX_ORDER_TOL = 5e-6  # tests/test_planar_round.py: identical rays, only the float summation order differs
FLUX_TOL = 1e-4        # ... and on the source-normalised flux
SEED = 12345
P, R = BC.PERIODIC_BOUNDARY, BC.REFLECTIVE_BOUNDARY
ORACLE_BC = {P: po.PERIODIC, R: po.REFLECTIVE}


@functools.lru_cache(maxsize=None)
def scene(name):
    """points, normals (read-only arrays), gridDelta, the number of rays, the source direction and the boundary conditions"""
    n1, n2, rays = (64, 64, 4_000_000) if name == "g" else (32, 48, 200_000) if name == "r" else (32, 32, 200_000)
    delta = 0.5 if name == "p" else 1.0
    x0 = 0.37 if name == "s" else -(n1 - 1) / 2.0 * delta
    y0 = 0.37 if name == "s" else -(n2 - 1) / 2.0 * delta
    X, Y = np.meshgrid(x0 + delta * np.arange(n1), y0 + delta * np.arange(n2), indexing="ij")
    X, Y = X.ravel().copy(), Y.ravel().copy()
    if name == "j":  # every centre off its lattice point by up to 0.05 delta per axis
        rng = np.random.default_rng(20240611)
        X += rng.uniform(-0.05, 0.05, X.size) * delta
        Y += rng.uniform(-0.05, 0.05, Y.size) * delta
    if name == "m":  # an interior disk moved by 0.3 delta along x
        X[13 * n2 + 17] += 0.3 * delta
    height = np.float32(0.3) if name == "f" else np.float32(0.0)
    pts = np.stack([X, Y, np.full(X.size, height)], -1).astype(np.float32)
    nrm = np.tile(np.array([0, 0, 1], np.float32), (len(pts), 1))
    direction = vr.TraceDirection.POS_Z
    bcs = {"b": (R, R, R), "c": (P, R, P)}.get(name, (P, P, P))
    if name == "d":  # a hole in the middle of the lattice
        i, j = np.meshgrid(np.arange(n1), np.arange(n2), indexing="ij")
        keep = ~((i >= 13) & (i < 19) & (j >= 13) & (j < 19)).ravel()
        assert keep.sum() == n1 * n2 - 36
        pts, nrm = pts[keep], nrm[keep]
    if name == "u":  # an interior disk twice
        pts = np.concatenate([pts, pts[13 * n2 + 17:13 * n2 + 18]])
        nrm = np.concatenate([nrm, nrm[:1]])
    if name == "f":
        pts = np.ascontiguousarray(pts[:, [2, 0, 1]])  # the plane x = 0.3f
        nrm = np.tile(np.array([1, 0, 0], np.float32), (len(pts), 1))
        direction = vr.TraceDirection.POS_X
    pts = np.ascontiguousarray(pts)
    nrm = np.ascontiguousarray(nrm)
    pts.setflags(write=False)
    nrm.setflags(write=False)
    return pts, nrm, delta, rays, direction, bcs


def gpu_run(name, knob, monkeypatch, capfd):
    monkeypatch.setenv("VR_SMALL_SCENE", "0")
    monkeypatch.setenv("VR_PLANAR_LATTICE", str(knob))
    monkeypatch.setenv("VR_PRINT_LAUNCHES", "1")
    pts, nrm, delta, rays, direction, bcs = scene(name)
    t = vr.TraceDisk(3)
    t.setGeometry(pts, nrm, delta)
    t.setBoundaryConditions(list(bcs))
    t.setSourceDirection(direction)
    t.setParticleType(vr.DiffuseParticle(1.0, "flux"))
    t.setNumberOfRaysFixed(rays)
    t.setRngSeed(SEED)
    capfd.readouterr()
    t.apply()
    err = capfd.readouterr().err
    rnd = re.search(r"\[vr\] planar disks: round: VR_PLANAR_ROUND (\d), launch (\d)", err)
    lat = re.search(r"\[vr\] planar disks: lattice: scene (\d), VR_PLANAR_LATTICE (\d), launch (\d)", err)
    assert rnd, "no planar-round line on stderr"
    assert lat, "no planar-lattice line on stderr"
    assert err.index("[vr] planar disks: round:") < err.index("[vr] planar disks: lattice:")  # the third line, after the two planar ones
    info = t.getRayTraceInfo()
    return {"t": t, "f32": t.getLocalData().getVectorData(0).copy(), "f64": t.getFluxF64(), "mode": t.traceMode(),
            "info": {k: int(getattr(info, k)) for k in COUNTERS}, "round": tuple(int(v) for v in rnd.groups()),
            "lattice": tuple(int(v) for v in lat.groups())}


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    pts, nrm, delta, rays, direction, bcs = scene(name)
    o = po.Oracle()
    o.set_disks(pts, nrm, delta, 3)
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
    assert ref.any()
    err = l2_rel(run["f32"], ref)
    print("  oracle L2", err, {k: oi[k] for k in ORACLE_COUNTERS})
    assert err <= FLUX_ORDER_TOL, err
    assert l2_rel(run["t"].normalizeFlux(run["f32"]), o.normalize_flux(ref)) <= FLUX_TOL


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "f", "g", "r", "p", "s", "j"])
def test_lattice_window_changes_no_result(name, monkeypatch, capfd):
    off = gpu_run(name, 0, monkeypatch, capfd)
    on = gpu_run(name, 1, monkeypatch, capfd)
    print(name, "modes", off["mode"], on["mode"], "round", off["round"], on["round"], "lattice", off["lattice"], on["lattice"], on["info"])
    assert off["mode"] == 1 and on["mode"] == 1  # (the flat absorbing kernel; the reported mode stays 1)
    assert off["round"] == (1, 1) and on["round"] == (1, 1)  # a one-point-per-round kernel ran both times
    assert off["lattice"] == (1, 0, 0)  # a lattice cloud; the knob forces the launch's flag false: the parent's kernel
    assert on["lattice"] == (1, 1, 1)
    assert on["info"] == off["info"], (off["info"], on["info"])
    i = on["info"]
    assert i["geometryHits"] > 0 and on["f64"].sum() > 0
    if name == "d":
        assert i["nonGeometryHits"] > 0, i  # rays through the hole
    if name in ("b", "c"):
        assert i["boundaryHits"] > 0, i
    assert np.array_equal(off["f64"], on["f64"])
    assert np.array_equal(off["f32"], on["f32"])
    against_oracle(name, off)
    against_oracle(name, on)


@pytest.mark.parametrize("name", ["m", "u"])
def test_not_a_lattice_cloud_keeps_the_parents_kernel(name, monkeypatch, capfd):
    run = gpu_run(name, 1, monkeypatch, capfd)
    print(name, "round", run["round"], "lattice", run["lattice"], run["info"])
    assert run["mode"] == 1
    assert run["round"] == (1, 1)  # still planar: the one-point-per-round kernel
    assert run["lattice"] == (0, 1, 0)  # the knob is on, the scene is no lattice cloud, the launch does not take the table
    assert run["info"]["geometryHits"] > 0
    against_oracle(name, run)
