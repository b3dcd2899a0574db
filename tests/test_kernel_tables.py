"""Each of the library's kernel tables (vr_kernel_table.hpp, generated from the catalogue of vr_types.hpp) really serves a
launch: one launch per mode a plain scene reaches, and for each of them traceMode() and the VR_PRINT_LAUNCHES lines name
the kernel asked for, every oracle counter equals the CPU oracle's and the flux agrees within the bounds of
tests/test_planar_round.py (L2-relative <= 5e-6: identical rays, only the float summation order differs; <= 1e-4 on the
source-normalised flux).

The scene is that of tests/test_planar_round.py: disks on a 32 x 32 lattice of pitch 1, periodic walls, 200 000 rays, seed
12345.  DiffuseParticle of sticking 1 runs MODE_ABSORB_FLAT (1) and, under VR_UNIFORM_DISKS / VR_PLANAR_DISKS /
VR_PLANAR_ROUND / VR_PLANAR_LATTICE / VR_LATTICE_LANE_TESTS, that mode's table entries 8 to 12 (with every knob at its
default the scene climbs the whole ladder: tests/test_lattice_lanes.py, scene "a"); VR_ABSORB_CARRY=1 gives MODE_ABSORB (2); sticking 0.5 runs
MODE_GENERAL_FLAT (3), with VR_GENERAL_FLAT=0 MODE_GENERAL (0), and with flux statistics the statistics table's
MODE_GENERAL_FLAT.  MODE_SMALL (4) runs on the 2-D trench of tests/golden/data (a few hundred disks).

The modes of a scene with relief are asserted where such scenes are built: MODE_ABSORB_RELIEF (5) and MODE_GENERAL_RELIEF
(6) with its loose launch in MODE_RESUME (7) by tests/test_gpu_parity.py::test_relief_packets_match_the_oracle, against the
oracle as well."""
import functools
import re

import numpy as np
import pytest

import viennaray_amd as vr
from viennaray_amd import BoundaryCondition as BC, TraceDirection as TD
from oracle import pyoracle as po
from helpers import l2_rel, trench2d

pytestmark = pytest.mark.gpu

ORACLE_COUNTERS = ("totalRaysTraced", "nonGeometryHits", "geometryHits", "boundaryHits", "reflections", "raysTerminated")
FLUX_ORDER_TOL = 5e-6  # tests/test_planar_round.py
FLUX_TOL = 1e-4        # ... and on the source-normalised flux
SEED, RAYS = 12345, 200_000
KNOBS = ("VR_UNIFORM_DISKS", "VR_PLANAR_DISKS", "VR_PLANAR_ROUND", "VR_PLANAR_LATTICE", "VR_LATTICE_LANE_TESTS", "VR_ABSORB_CARRY",
         "VR_GENERAL_FLAT")

# name: (scene, sticking, flux statistics, environment, traceMode(), the mode of the kernel launched)
CASES = {
    "general": ("lattice", 0.5, False, {"VR_GENERAL_FLAT": "0"}, 0, 0),
    "absorb_flat": ("lattice", 1.0, False, {"VR_UNIFORM_DISKS": "0"}, 1, 1),
    "absorb": ("lattice", 1.0, False, {"VR_ABSORB_CARRY": "1"}, 2, 2),
    "general_flat": ("lattice", 0.5, False, {}, 3, 3),
    "small": ("trench2d", 0.5, False, {}, 4, 4),
    "uniform": ("lattice", 1.0, False, {"VR_UNIFORM_DISKS": "1", "VR_PLANAR_DISKS": "0"}, 1, 8),
    "planar": ("lattice", 1.0, False, {"VR_UNIFORM_DISKS": "1", "VR_PLANAR_DISKS": "1", "VR_PLANAR_ROUND": "0"}, 1, 9),
    "planar_round": ("lattice", 1.0, False, {"VR_UNIFORM_DISKS": "1", "VR_PLANAR_DISKS": "1", "VR_PLANAR_ROUND": "1",
                                             "VR_PLANAR_LATTICE": "0"}, 1, 10),
    "lattice": ("lattice", 1.0, False, {"VR_PLANAR_LATTICE": "1", "VR_LATTICE_LANE_TESTS": "0"}, 1, 11),
    "lattice_lanes": ("lattice", 1.0, False, {}, 1, 12),
    "statistics_general_flat": ("lattice", 0.5, True, {}, 3, 3),
    "statistics_small": ("trench2d", 0.5, True, {}, 4, 4),
}


@functools.lru_cache(maxsize=None)
def scene(name):
    """points, normals (read-only), grid delta, dimension, source direction, boundary conditions"""
    if name == "trench2d":
        gd, pts, nrm = trench2d()
        out = (np.ascontiguousarray(pts), np.ascontiguousarray(nrm), gd, 2, TD.POS_Y, (BC.REFLECTIVE_BOUNDARY,) * 2)
    else:
        n = 32
        x0 = -(n - 1) / 2.0
        X, Y = np.meshgrid(x0 + np.arange(n), x0 + np.arange(n), indexing="ij")
        pts = np.ascontiguousarray(np.stack([X.ravel(), Y.ravel(), np.zeros(n * n)], -1).astype(np.float32))
        nrm = np.ascontiguousarray(np.tile(np.array([0, 0, 1], np.float32), (n * n, 1)))
        out = (pts, nrm, 1.0, 3, TD.POS_Z, (BC.PERIODIC_BOUNDARY,) * 3)
    out[0].setflags(write=False)
    out[1].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_run(name, sticking):
    pts, nrm, gd, D, direction, bcs = scene(name)
    o = po.Oracle()
    o.set_disks(pts, nrm, gd, D)
    o.set_boundary_conditions([int(b) for b in bcs])
    o.set_source_direction(int(direction))
    o.set_particle(po.DIFFUSE, sticking)
    o.set_num_rays_fixed(RAYS)
    o.set_rng_seed(SEED)
    o.set_lazy_rng(True)
    o.apply(po.max_threads())
    return o, o.flux(), o.info()


def kernel_mode(trace_mode, err):
    """the mode of the kernel the launch ran (ParticleLaunch::kernelMode), from the VR_PRINT_LAUNCHES line that names it;
    the five lines of the absorbing flat-scene ladder say the same, rung by rung"""
    m = re.search(r"\[vr\] kernel: traceMode (\d+), kernel mode (\d+), particle 0", err)
    assert m, "no kernel line on stderr"
    assert int(m.group(1)) == trace_mode
    kernel = int(m.group(2))
    launched = {}
    for key, pattern in (("uniform", r"\[vr\] uniform disks: scene \d, VR_UNIFORM_DISKS \d, launch (\d)"),
                         ("planar", r"\[vr\] planar disks: scene \d, VR_PLANAR_DISKS \d, launch (\d)"),
                         ("round", r"\[vr\] planar disks: round: VR_PLANAR_ROUND \d, launch (\d)"),
                         ("lattice", r"\[vr\] planar disks: lattice: scene \d, VR_PLANAR_LATTICE \d, launch (\d)"),
                         ("lanes", r"\[vr\] planar disks: lanes: scene \d, VR_LATTICE_LANE_TESTS \d, launch (\d)")):
        m = re.search(pattern, err)
        assert m, "no %s line on stderr" % key
        launched[key] = int(m.group(1))
    assert launched["lanes"] <= launched["lattice"] <= launched["round"] <= launched["planar"] <= launched["uniform"], launched
    if launched["uniform"]:
        assert trace_mode == 1, (trace_mode, launched)
    assert kernel == (7 + sum(launched.values()) if launched["uniform"] else trace_mode), (kernel, trace_mode, launched)
    return kernel


@pytest.mark.parametrize("name", list(CASES))
def test_the_table_serves_the_launch(name, monkeypatch, capfd):
    which, sticking, stats, env, mode, kernel = CASES[name]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if which == "lattice":
        monkeypatch.setenv("VR_SMALL_SCENE", "0")
    monkeypatch.setenv("VR_PRINT_LAUNCHES", "1")
    pts, nrm, gd, D, direction, bcs = scene(which)
    t = vr.TraceDisk(D)
    t.setGeometry(pts, nrm, gd)
    t.setBoundaryConditions(list(bcs))
    t.setSourceDirection(direction)
    t.setParticleType(vr.DiffuseParticle(sticking, "flux"))
    t.setNumberOfRaysFixed(RAYS)
    t.setRngSeed(SEED)
    if stats:
        t.setCalculateFluxError(True)
    capfd.readouterr()
    t.apply()
    err = capfd.readouterr().err
    got_mode, got_kernel = t.traceMode(), kernel_mode(t.traceMode(), err)
    info = t.getRayTraceInfo()
    got = {k: int(getattr(info, k)) for k in ORACLE_COUNTERS}
    o, ref, oi = oracle_run(which, sticking)
    flux = t.getLocalData().getVectorData(0)
    l2 = l2_rel(flux, ref)
    print(name, "traceMode", got_mode, "kernel", got_kernel, "oracle L2", l2, got)
    assert (got_mode, got_kernel) == (mode, kernel)
    assert got == {k: oi[k] for k in ORACLE_COUNTERS}, (got, oi)
    assert got["geometryHits"] > 0 and ref.any()
    assert l2 <= FLUX_ORDER_TOL, l2
    assert l2_rel(t.normalizeFlux(flux), o.normalize_flux(ref)) <= FLUX_TOL
