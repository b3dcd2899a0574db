"""The generator's sort-bin grid aligned with the disk lattice (VR_BIN_ALIGN, vr_bin_grid.hpp) only orders the work:
every case runs once with VR_BIN_ALIGN=0 and once with =1 — both set before the tracer is made, the LDS-resident
small-scene kernel off — and the raw flux arrays are equal element for element, as is every TraceInfo counter.  One case
per scene also goes against the CPU oracle with the bounds of tests/test_flat_absorbing_scalar.py (counters equal, flux
L2-relative error <= 5e-6, <= 1e-4 on the source-normalised flux).

The scenes are the smallest that reach each branch of the rule and of the key: one partial tile (plane_grid(9)), several
tiles (plane_grid(40)), T1 != T2 with a partial tile on each axis (40 x 24), a pitch and a phase that are not trivial
(32 x 32 of pitch 0.7 from (0.3, -1.1)), a cloud that is no lattice, the trench (structured-scene kernels), and the two
whose grid must stay the plain one: the rippled plane (bin_of_relief through the shared key helper; relief launches
measured slower with the aligned grid and keep the plain one) and a line of disks in two dimensions.  2 000, 20 000 and
200 000 rays on the 40 x 40 plane are 1.3, 13 and 130 rays per lattice cell: the rule's sparse branch with several cells
per bin along both axes, its sparse branch with one cell along the second axis, and its dense branch with a cut cell.
The 3-D disk cases assert that the second run's grid IS the aligned one (the VR_PRINT_LAUNCHES line)."""
import re

import numpy as np
import pytest

import viennaray_amd as vr
from viennaray_amd import BoundaryCondition as BC, TraceDirection as TD
from oracle import pyoracle as po
from helpers import l2_rel, trench3d

pytestmark = pytest.mark.gpu

COUNTERS = ("numRays", "totalRaysTraced", "nonGeometryHits", "geometryHits", "particleHits", "boundaryHits", "reflections",
            "raysTerminated", "rngFullStates")
ORACLE_COUNTERS = ("totalRaysTraced", "nonGeometryHits", "geometryHits", "boundaryHits", "reflections", "raysTerminated")
FLUX_ORDER_TOL = 5e-6  # tests/test_flat_absorbing_scalar.py: identical rays, only the float summation order differs
FLUX_TOL = 1e-4        # ... and on the source-normalised flux
RANGE = (12_345, 77_777)  # starts inside a 64-ray packet and ends inside another one
PER, REF = BC.PERIODIC_BOUNDARY, BC.REFLECTIVE_BOUNDARY


def lattice(nx, ny, pitch=1.0, x0=None, y0=None):
    """nx x ny disks of the given pitch on the plane z = 0, normals +z, the first centre at (x0, y0)"""
    x0 = -(nx - 1) / 2.0 * pitch if x0 is None else x0
    y0 = -(ny - 1) / 2.0 * pitch if y0 is None else y0
    X, Y = np.meshgrid(x0 + np.arange(nx) * pitch, y0 + np.arange(ny) * pitch, indexing="ij")
    pts = np.stack([X.ravel(), Y.ravel(), np.zeros(nx * ny)], -1).astype(np.float32)
    return pts, np.tile(np.array([0, 0, 1], np.float32), (nx * ny, 1))


def rippled_plane(n=40):
    """plane_grid(n) with half a grid cell of relief (tests/test_flat_absorbing_scalar.py, the benchmark's C2_rippled)"""
    pts, _ = vr.io.plane_grid(n, 1.0)
    x, y = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    amp, wave = 0.5, 4.0
    pts = pts.copy()
    pts[:, 2] = (amp * np.sin(x / wave) * np.cos(y / wave)).astype(np.float32)
    nv = np.stack([-amp / wave * np.cos(x / wave) * np.cos(y / wave), amp / wave * np.sin(x / wave) * np.sin(y / wave),
                   np.ones_like(x)], -1)
    return pts, (nv / np.linalg.norm(nv, axis=1, keepdims=True)).astype(np.float32)


def scene(name):
    """points, normals, gridDelta, D, source direction"""
    if name in ("plane9", "plane40"):
        return vr.io.plane_grid(int(name[5:]), 1.0) + (1.0, 3, TD.POS_Z)
    if name == "lat40x24":
        return lattice(40, 24) + (1.0, 3, TD.POS_Z)
    if name == "pitch0.7":
        return lattice(32, 32, 0.7, 0.3, -1.1) + (0.7, 3, TD.POS_Z)
    if name == "ripple40":
        return rippled_plane(40) + (1.0, 3, TD.POS_Z)
    if name == "jitter32":
        pts, nrm = vr.io.plane_grid(32, 1.0)
        pts = pts.copy()
        pts[:, :2] += ((np.random.default_rng(7).random((len(pts), 2)) * 2 - 1) * 0.3).astype(np.float32)
        return pts, nrm, 1.0, 3, TD.POS_Z
    if name == "trench3d":
        gd, p, n = trench3d()
        return p, n, gd, 3, TD.POS_Z
    assert name == "line17"
    pts = np.zeros((17, 3), np.float32)
    pts[:, 0] = np.arange(17) - 8.0
    return pts, np.tile(np.array([0, 1, 0], np.float32), (17, 1)), 1.0, 2, TD.POS_Y


def gpu_run(name, bc, sticking, rays, ray_range, align, extra, monkeypatch, capfd):
    monkeypatch.setenv("VR_SMALL_SCENE", "0")
    monkeypatch.setenv("VR_BIN_ALIGN", str(align))
    monkeypatch.setenv("VR_PRINT_LAUNCHES", "1")
    if extra:
        monkeypatch.setenv(*extra)
    pts, nrm, gd, D, direction = scene(name)
    t = vr.TraceDisk(D)
    t.setGeometry(pts, nrm, gd)
    t.setBoundaryConditions([bc] * D)
    t.setSourceDirection(direction)
    t.setParticleType(vr.DiffuseParticle(sticking, "flux"))
    t.setNumberOfRaysFixed(rays)
    t.setRngSeed(4711)
    if ray_range:
        t.setRayRange(*ray_range)
    capfd.readouterr()
    t.apply()
    line = re.search(r"\[vr\] sort bins: (\d+) \((\d+) x (\d+) cells\), VR_BIN_ALIGN (\d), aligned (\d), cell (\S+) x (\S+) gridDelta",
                     capfd.readouterr().err)
    assert line, "no sort-bin line on stderr"
    info = t.getRayTraceInfo()
    return {"t": t, "f32": t.getLocalData().getVectorData(0).copy(), "f64": t.getFluxF64(), "mode": t.traceMode(),
            "info": {k: int(getattr(info, k)) for k in COUNTERS}, "bins": int(line.group(1)), "knob": int(line.group(4)),
            "aligned": int(line.group(5)), "cells": (int(line.group(2)), int(line.group(3))),
            "cell": (float(line.group(6)), float(line.group(7)))}


def oracle_run(name, bc, rays, ray_range):
    pts, nrm, gd, D, direction = scene(name)
    o = po.Oracle()
    o.set_disks(pts, nrm, gd, D)
    o.set_boundary_conditions([int(bc)] * D)
    o.set_source_direction(int(direction))
    o.set_particle(po.DIFFUSE, 1.0)
    o.set_num_rays_fixed(rays)
    o.set_rng_seed(4711)
    if ray_range:
        o.set_ray_range(*ray_range)
    o.set_lazy_rng(True)
    o.apply(po.max_threads())
    return o, o.flux(), o.info()


# (scene, walls, sticking, rays, ray range, extra knob, trace mode, against the oracle, the aligned cell in gridDelta or None)
CASES = [
    ("plane9", PER, 1.0, 200_000, None, None, 1, True, None),
    ("plane40", PER, 1.0, 200_000, None, None, 1, True, (1.0, 1.0 / 3.0)),
    ("plane40", REF, 1.0, 200_000, None, None, 1, False, None),
    ("plane40", PER, 1.0, 20_000, None, None, 1, False, (3.0, 1.0)),
    ("plane40", REF, 1.0, 2_000, None, None, 1, False, (6.0, 5.0)),
    ("plane40", PER, 0.1, 200_000, None, None, 3, False, None),
    ("plane40", REF, 1.0, 200_000, RANGE, None, 1, False, None),
    ("plane40", PER, 1.0, 200_000, None, ("VR_BATCH_RAYS", "65536"), 1, False, None),
    # a last batch whose own aligned grid would have MORE bins than the one the buffers were sized for (4 000 rays: 5 x 3 cells,
    # 128 bins; 3 750 rays: 4 x 4, 256 bins — vr_bin_grid.hpp's rule on an extent of 39): it keeps the sized grid
    ("plane40", PER, 1.0, 7_750, None, ("VR_BATCH_RAYS", "4000"), 1, False, (5.0, 3.0)),
    ("lat40x24", PER, 1.0, 200_000, None, None, 1, True, None),
    ("lat40x24", REF, 0.1, 200_000, None, None, 3, False, None),
    ("pitch0.7", PER, 1.0, 200_000, None, None, 1, True, None),
    ("pitch0.7", REF, 0.1, 200_000, None, None, 3, False, None),
    ("ripple40", PER, 1.0, 200_000, None, None, 5, True, None),
    ("ripple40", REF, 0.1, 200_000, None, None, 6, False, None),
    ("jitter32", PER, 1.0, 200_000, None, None, 1, True, None),
    ("trench3d", PER, 1.0, 200_000, None, None, 2, True, None),
    ("trench3d", REF, 0.1, 200_000, None, None, 0, False, None),
    ("line17", PER, 1.0, 200_000, None, None, 1, True, None),
    ("line17", REF, 0.1, 200_000, None, None, 3, False, None),
]


def case_id(c):
    return "-".join([c[0], "per" if c[1] == PER else "ref", "s%g" % c[2], "%dk" % (c[3] // 1000)] + (["range"] if c[4] else []) +
                    (["batches"] if c[5] else []))


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_aligned_bins_change_no_result(case, monkeypatch, capfd):
    name, bc, sticking, rays, ray_range, extra, mode, oracle, cell = case
    a = gpu_run(name, bc, sticking, rays, ray_range, 0, extra, monkeypatch, capfd)
    b = gpu_run(name, bc, sticking, rays, ray_range, 1, extra, monkeypatch, capfd)
    print(case_id(case), "modes", a["mode"], b["mode"], "bins", a["bins"], a["cells"], "->", b["bins"], b["cells"], "cell", b["cell"],
          "aligned", a["aligned"], b["aligned"], b["info"])
    assert a["mode"] == mode and b["mode"] == mode, (a["mode"], b["mode"])
    assert (a["knob"], b["knob"]) == (0, 1)
    assert a["aligned"] == 0
    if name in ("line17", "ripple40"):  # two dimensions, and a scene with relief (measured slower aligned): the plain grid, whatever the knob
        assert b["aligned"] == 0 and b["bins"] == a["bins"] and b["cells"] == a["cells"]
    else:
        assert b["aligned"] == 1
        # whole lattice cells along the first axis, m cells or 1 / k of one along the second
        m1, c2 = b["cell"]
        assert abs(m1 - round(m1)) < 1e-3 and (abs(c2 - round(c2)) < 1e-3 or abs(1 / c2 - round(1 / c2)) < 1e-2), b["cell"]
        if cell:
            assert b["cell"] == pytest.approx(cell, rel=1e-3)
    assert b["info"] == a["info"], (a["info"], b["info"])
    assert b["info"]["geometryHits"] > 0 and a["f64"].sum() > 0
    assert np.array_equal(a["f64"], b["f64"])
    assert np.array_equal(a["f32"], b["f32"])
    if oracle:
        o, r, oi = oracle_run(name, bc, rays, ray_range)
        err = l2_rel(b["f32"], r)
        print("  oracle L2", err)
        assert {k: b["info"][k] for k in ORACLE_COUNTERS} == {k: oi[k] for k in ORACLE_COUNTERS}, (b["info"], oi, err)
        assert err <= FLUX_ORDER_TOL, err
        assert l2_rel(b["t"].normalizeFlux(b["f32"]), o.normalize_flux(r)) <= FLUX_TOL
