"""The lattice cloud's kernel with four disk tests per lane in place of the candidate loop (VR_LATTICE_LANE_TESTS;
MODE_ABSORB_FLAT_LATTICE_LANES, pq_hit_lattice_lanes, vr_planar_lattice.hpp "four corners per lane"): where the disks are small
enough against the pitch, only the lattice points at the corners of a ray's own cell can accept its plane point, so each
lane tests those four and credits them through the wave's LDS counters.  Same rays, same acceptance arithmetic, integer
sums: every scene runs once with VR_LATTICE_LANE_TESTS=0 (MODE_ABSORB_FLAT_LATTICE as it was) and once with =1, both with
VR_SMALL_SCENE=0, and the raw float32 and float64 flux arrays are equal element for element, as is every TraceInfo counter;
each run also goes against the CPU oracle with the bounds of tests/test_planar_lattice.py (counters equal, flux L2-relative
error <= 5e-6, <= 1e-4 on the source-normalised flux).  The VR_PRINT_LAUNCHES lines say which kernel the launch ran.
A round whose window of lattice cells does not fit the wave (rays folded in from the far side by periodic or reflective
walls) takes the kernel's direct form with the knob on — each lane its four table words and records from global memory —
and the tree packet and the walk with it off: the same comparison covers the direct form against its fall-back.

The scenes: (a) (b) (c) (d) (f) (g) (r) (p) (s) (j) of tests/test_planar_lattice.py, and (k) every centre jittered by up to
0.12 gridDelta per axis, seeded; (t) a 2 x 3 lattice under 50 000 rays with reflective walls: every corner lookup meets a
table edge; (h) scene (d) with a 16 x 16 hole: whole windows are empty.  Two scenes keep MODE_ABSORB_FLAT_LATTICE and still
match the oracle: (o) a 32 x 32 lattice moved so far from the origin that the host rule refuses it — the offset is what
tests/aux/lattice_lanes.cpp computes from the rule, for this pitch and radius — and (m) that file's cloud with one centre
0.3 gridDelta off, which is no lattice cloud at all."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import viennaray_amd as vr
from viennaray_amd import BoundaryCondition as BC
from oracle import pyoracle as po
from helpers import l2_rel
import test_planar_lattice as base

pytestmark = pytest.mark.gpu

COUNTERS = base.COUNTERS
ORACLE_COUNTERS = base.ORACLE_COUNTERS
FLUX_ORDER_TOL = 5e-6  # tests/test_planar_lattice.py: identical rays, only the float summation order differs
FLUX_TOL = 1e-4        # ... and on the source-normalised flux
SEED = 12345
P, R = BC.PERIODIC_BOUNDARY, BC.REFLECTIVE_BOUNDARY
ORACLE_BC = {P: po.PERIODIC, R: po.REFLECTIVE}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE_SCENES = ("a", "b", "c", "d", "f", "g", "r", "p", "s", "j", "m")


@functools.lru_cache(maxsize=None)
def refusing_offset(tmp):
    """the smallest power-of-two offset at which the host rule refuses a 32 x 32 lattice of pitch 1 (the host program's)"""
    pts, nrm, delta, _, _, _ = base.scene("a")
    t = vr.TraceDisk(3)
    t.setGeometry(pts, nrm, delta)
    radius = float(t.getDiskRadius())
    exe = os.path.join(tmp, "lattice_lanes")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I", os.path.join(ROOT, "viennaray_amd", "csrc"),
                           os.path.join(ROOT, "tests", "aux", "lattice_lanes.cpp"), "-o", exe])
    out = subprocess.run([exe, "offset", repr(delta), "%.9g" % radius, "32"], capture_output=True, text=True, timeout=60, check=True)
    off = float(out.stdout)
    assert 1.0 <= off <= 2.0 ** 20 and np.float32(off) == off, out.stdout
    return off


@functools.lru_cache(maxsize=None)
def scene(name, offset=0.0):
    """points, normals (read-only arrays), gridDelta, the number of rays, the source direction and the boundary conditions"""
    if name in BASE_SCENES:
        return base.scene(name)
    n1, n2, rays = (2, 3, 50_000) if name == "t" else (32, 32, 200_000)
    delta = 1.0
    x0, y0 = -(n1 - 1) / 2.0 * delta + offset, -(n2 - 1) / 2.0 * delta + offset
    if name == "o":  # the first centre AT the offset: every coordinate at or beyond it
        assert offset > 0.0
        x0 = y0 = offset
    X, Y = np.meshgrid(x0 + delta * np.arange(n1), y0 + delta * np.arange(n2), indexing="ij")
    X, Y = X.ravel().copy(), Y.ravel().copy()
    if name == "k":  # every centre off its lattice point by up to 0.12 delta per axis (the table takes delta / 8)
        rng = np.random.default_rng(20250117)
        jx, jy = rng.uniform(-0.12, 0.12, (n1, n2)), rng.uniform(-0.12, 0.12, (n1, n2))
        # (the lattice's phase is the smallest centre coordinate: the first column / row stays at or above its line, one
        #  disk on it, so that the 0.12 is measured from the lattice the table is built on)
        jx[0, :], jy[:, 0] = np.abs(jx[0, :]), np.abs(jy[:, 0])
        jx[0, 0] = jy[0, 0] = 0.0
        X += jx.ravel() * delta
        Y += jy.ravel() * delta
    pts = np.stack([X, Y, np.zeros(X.size)], -1).astype(np.float32)
    if name == "h":  # a hole of 16 x 16 lattice points: rounds over it find whole windows empty
        i, j = np.meshgrid(np.arange(n1), np.arange(n2), indexing="ij")
        keep = ~((i >= 8) & (i < 24) & (j >= 8) & (j < 24)).ravel()
        assert keep.sum() == n1 * n2 - 256
        pts = pts[keep]
    pts = np.ascontiguousarray(pts)
    nrm = np.ascontiguousarray(np.tile(np.array([0, 0, 1], np.float32), (len(pts), 1)))
    pts.setflags(write=False)
    nrm.setflags(write=False)
    return pts, nrm, delta, rays, vr.TraceDirection.POS_Z, (R, R, R) if name == "t" else (P, P, P)


def gpu_run(sc, knob, monkeypatch, capfd):
    monkeypatch.setenv("VR_SMALL_SCENE", "0")
    monkeypatch.setenv("VR_LATTICE_LANE_TESTS", str(knob))
    monkeypatch.setenv("VR_PRINT_LAUNCHES", "1")
    pts, nrm, delta, rays, direction, bcs = sc
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
    lan = re.search(r"\[vr\] planar disks: lanes: scene (\d), VR_LATTICE_LANE_TESTS (\d), launch (\d), particle \d+\n", err)
    assert rnd and lat, "no planar-round / planar-lattice line on stderr"
    assert lan, "no lanes line on stderr"
    assert err.index("[vr] planar disks: lattice:") < err.index("[vr] planar disks: lanes:")  # the fourth line, after the three
    info = t.getRayTraceInfo()
    return {"t": t, "f32": t.getLocalData().getVectorData(0).copy(), "f64": t.getFluxF64(), "mode": t.traceMode(),
            "info": {k: int(getattr(info, k)) for k in COUNTERS}, "round": tuple(int(v) for v in rnd.groups()),
            "lattice": tuple(int(v) for v in lat.groups()), "lanes": tuple(int(v) for v in lan.groups())}


@functools.lru_cache(maxsize=None)
def oracle_run(name, offset=0.0):
    if name in BASE_SCENES:  # (one reference per scene for both files)
        return base.oracle_run(name)
    pts, nrm, delta, rays, direction, bcs = scene(name, offset)
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


def against_oracle(run, oracle):
    o, ref, oi = oracle
    assert {k: run["info"][k] for k in ORACLE_COUNTERS} == {k: oi[k] for k in ORACLE_COUNTERS}, (run["info"], oi)
    assert ref.any()
    err = l2_rel(run["f32"], ref)
    print("  oracle L2", err, {k: oi[k] for k in ORACLE_COUNTERS})
    assert err <= FLUX_ORDER_TOL, err
    assert l2_rel(run["t"].normalizeFlux(run["f32"]), o.normalize_flux(ref)) <= FLUX_TOL


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "f", "g", "r", "p", "s", "j", "k", "t", "h"])
def test_four_lane_tests_change_no_result(name, monkeypatch, capfd):
    sc = scene(name)
    off = gpu_run(sc, 0, monkeypatch, capfd)
    on = gpu_run(sc, 1, monkeypatch, capfd)
    print(name, "modes", off["mode"], on["mode"], "lattice", off["lattice"], on["lattice"], "lanes", off["lanes"], on["lanes"], on["info"])
    assert off["mode"] == 1 and on["mode"] == 1  # (the flat absorbing kernel; the reported mode stays 1)
    assert off["round"] == (1, 1) and on["round"] == (1, 1)
    assert off["lattice"] == (1, 1, 1) and on["lattice"] == (1, 1, 1)  # a lattice cloud's kernel ran both times ...
    assert off["lanes"] == (1, 0, 0)  # ... the rule holds; the knob forces the launch's flag false: MODE_ABSORB_FLAT_LATTICE
    assert on["lanes"] == (1, 1, 1)   # ... MODE_ABSORB_FLAT_LATTICE_LANES
    assert on["info"] == off["info"], (off["info"], on["info"])
    i = on["info"]
    assert i["geometryHits"] > 0 and on["f64"].sum() > 0
    if name in ("d", "h"):
        assert i["nonGeometryHits"] > 0, i  # rays through the hole
    if name in ("b", "c", "t"):
        assert i["boundaryHits"] > 0, i
    assert np.array_equal(off["f64"], on["f64"])
    assert np.array_equal(off["f32"], on["f32"])
    against_oracle(off, oracle_run(name))
    against_oracle(on, oracle_run(name))


def test_far_from_the_origin_the_rule_refuses(monkeypatch, capfd, tmp_path_factory):
    offset = refusing_offset(str(tmp_path_factory.mktemp("lattice_lanes")))
    run = gpu_run(scene("o", offset), 1, monkeypatch, capfd)
    print("o: offset", offset, "round", run["round"], "lattice", run["lattice"], "lanes", run["lanes"], run["info"])
    assert run["mode"] == 1
    assert run["lattice"][0] == 1  # still a lattice cloud
    assert run["lanes"] == (0, 1, 0)  # the knob is on, the rule refuses the scene, the launch keeps MODE_ABSORB_FLAT_LATTICE
    assert run["info"]["geometryHits"] > 0
    against_oracle(run, oracle_run("o", offset))


def test_not_a_lattice_cloud_keeps_the_parents_kernel(monkeypatch, capfd):
    run = gpu_run(scene("m"), 1, monkeypatch, capfd)
    print("m: round", run["round"], "lattice", run["lattice"], "lanes", run["lanes"], run["info"])
    assert run["mode"] == 1
    assert run["round"] == (1, 1)  # still planar: the one-point-per-round kernel
    assert run["lattice"] == (0, 1, 0) and run["lanes"] == (0, 1, 0)
    assert run["info"]["geometryHits"] > 0
    against_oracle(run, oracle_run("m"))
