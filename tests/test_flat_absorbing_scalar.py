"""The absorbing flat-scene kernel (trace_kernel MODE 1, and MODE 5 on a plane with relief) against the CPU oracle on
the shapes where its wave-uniform bookkeeping can go wrong: one 8 x 8 tile of bins owned by a single span, a partial
tile (the boustrophedon order of the bins meets the edge), several tile rows, and a flat line of disks in two
dimensions — each with periodic and with reflective walls, as a whole launch and as a ray range whose last packet
round is partly filled.

Every TraceInfo counter is equal to the oracle's; the flux is held to the bounds of the MODE 1 parity tests of
tests/test_gpu_parity.py (`compare`: L2-relative error <= 5e-6, i.e. float summation order only, and <= 1e-4 on the
source-normalised flux).  The scenes are small enough for the LDS-resident kernel (MODE 4), which is switched off so
that the kernel under test runs: each case asserts the mode."""
import numpy as np
import pytest

import viennaray_amd as vr
from viennaray_amd import BoundaryCondition as BC, TraceDirection as TD
from oracle import pyoracle as po
from helpers import l2_rel

pytestmark = pytest.mark.gpu

RAYS = 200_000
COUNTERS = ("totalRaysTraced", "nonGeometryHits", "geometryHits", "boundaryHits", "reflections", "raysTerminated")
FLUX_ORDER_TOL = 5e-6  # test_gpu_parity.compare: identical rays, only the float summation order differs
FLUX_TOL = 1e-4        # ... and the north-star bound, on the source-normalised flux
# a range that starts inside a 64-ray packet and ends inside another one
RANGE = (12_345, 77_777)


def flat_line(n=17, gd=1.0):
    """n disks on the x axis, normals +y: a flat scene in two dimensions"""
    pts = np.zeros((n, 3), np.float32)
    pts[:, 0] = (np.arange(n) - (n - 1) / 2.0) * gd
    nrm = np.tile(np.array([0, 1, 0], np.float32), (n, 1))
    return pts, nrm


def rippled_plane(n=40):
    """plane_grid(n) with half a grid cell of relief: the formula of the benchmark's C2_rippled"""
    pts, _ = vr.io.plane_grid(n, 1.0)
    x, y = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    amp, wave = 0.5, 4.0
    pts = pts.copy()
    pts[:, 2] = (amp * np.sin(x / wave) * np.cos(y / wave)).astype(np.float32)
    nv = np.stack([-amp / wave * np.cos(x / wave) * np.cos(y / wave), amp / wave * np.sin(x / wave) * np.sin(y / wave),
                   np.ones_like(x)], -1)
    nrm = (nv / np.linalg.norm(nv, axis=1, keepdims=True)).astype(np.float32)
    return pts, nrm


def scene(shape):
    """points, normals, D, source direction"""
    if shape == "line17":
        return flat_line() + (2, TD.POS_Y)
    if shape == "ripple40":
        return rippled_plane(40) + (3, TD.POS_Z)
    return vr.io.plane_grid({"tile8": 8, "partial9": 9, "rows40": 40}[shape], 1.0) + (3, TD.POS_Z)


def oracle_run(shape, bc, ray_range):
    """flux and counters of the oracle for one case"""
    pts, nrm, D, direction = scene(shape)
    o = po.Oracle()
    o.set_disks(pts, nrm, 1.0, D)
    o.set_boundary_conditions([int(bc)] * D)
    o.set_source_direction(int(direction))
    o.set_particle(po.DIFFUSE, 1.0)
    o.set_num_rays_fixed(RAYS)
    o.set_rng_seed(4711)
    if ray_range:
        o.set_ray_range(*ray_range)
    o.set_lazy_rng(True)
    o.apply(po.max_threads())
    return o, o.flux(), o.info()


def check(shape, bc, ray_range, mode, monkeypatch):
    monkeypatch.setenv("VR_SMALL_SCENE", "0")  # (the scene from HBM: not the LDS-resident kernel)
    pts, nrm, D, direction = scene(shape)
    t = vr.TraceDisk(D)
    t.setGeometry(pts, nrm, 1.0)
    t.setBoundaryConditions([bc] * D)
    t.setSourceDirection(direction)
    t.setParticleType(vr.DiffuseParticle(1.0, "flux"))
    t.setNumberOfRaysFixed(RAYS)
    t.setRngSeed(4711)
    if ray_range:
        t.setRayRange(*ray_range)
    t.apply()
    assert t.traceMode() == mode, t.traceMode()
    f = t.getLocalData().getVectorData(0)
    info = t.getRayTraceInfo()
    o, r, oi = oracle_run(shape, bc, ray_range)
    err = l2_rel(f, r)
    got = {k: int(getattr(info, k)) for k in COUNTERS}
    print(shape, bc, ray_range, "mode", t.traceMode(), "L2", err, got)
    assert got == {k: oi[k] for k in COUNTERS}, (got, oi, err)
    assert oi["geometryHits"] > 0 and r.sum() > 0
    assert err <= FLUX_ORDER_TOL, err
    assert l2_rel(t.normalizeFlux(f), o.normalize_flux(r)) <= FLUX_TOL


@pytest.mark.parametrize("ray_range", [None, RANGE], ids=["whole", "range"])
@pytest.mark.parametrize("bc", [BC.PERIODIC_BOUNDARY, BC.REFLECTIVE_BOUNDARY], ids=["periodic", "reflective"])
@pytest.mark.parametrize("shape", ["tile8", "partial9", "rows40", "line17"])
def test_absorbing_flat_scene_matches_oracle(shape, bc, ray_range, monkeypatch):
    check(shape, bc, ray_range, 1, monkeypatch)


def test_absorbing_rippled_plane_matches_oracle(monkeypatch):
    """plane_grid(40) rippled by half a grid cell: the absorbing relief kernel (MODE 5)"""
    check("ripple40", BC.PERIODIC_BOUNDARY, None, 5, monkeypatch)
