"""Planar disks (VR_PLANAR_DISKS; pq_hit_packet PLANAR, vr_packet_query.hpp, vr_planar_disks.hpp): where the uniform disks of
a scene also share a plane normal to a coordinate axis, the 3-D absorbing flat-scene kernel computes the point where a
ray crosses that plane once per round and tests a distance per candidate.  That only removes repeated work: every case
that takes the variant runs once with VR_PLANAR_DISKS=1 and once with =0 (the uniform-disk kernel), and the raw float32
and float64 flux arrays are equal element for element, as is every TraceInfo counter; each case also goes against the
CPU oracle with the bounds of tests/test_uniform_disks.py (counters equal, flux L2-relative error <= 5e-6, <= 1e-4 on the
source-normalised flux).  The two VR_PRINT_LAUNCHES lines say what the scene is and which kernel the launch ran.

The scenes: disks on a 32 x 32 lattice of pitch 1, periodic walls, 200 000 rays, seed 12345, DiffuseParticle of
sticking 1 — (a) z = 0, normals (0, 0, 1); (b) z = 0.3f, normals (-0, 0, 1); (c) as (b) with one interior disk's z one
ulp higher: not planar, still uniform, the launch runs the uniform-disk kernel; (d) the tilted shared normal of
test_uniform_disks' scene "b": not planar; (e) a 64 x 64 lattice under 4 000 000 rays: full waves, several leaf nodes per
query; (f) normals (0, 0, -1) under the same source: the s = -1 path, every disk is met from behind and the neighbour test
credits nothing; (g) the plane x = 0.3f with normals (1, 0, 0) under a source along x: another axis; (h) as (f) with the
source on the other side (NEG_Z): s = -1 with hits that count and credit.

On (f): a disk met from behind is no geometry hit of the reference (rayTraceKernel.hpp:223-240: the ray goes on behind
the disk and leaves the scene), so `geometryHits` is 0 there for every kernel and for the oracle.  The hit test did accept:
each such hit starts one more segment, and the case asserts that count (totalRaysTraced - numRays - boundaryHits > 0) in
place of `geometryHits > 0`; (h) has `geometryHits > 0` on the same normals."""
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
FLUX_ORDER_TOL = 5e-6  # tests/test_uniform_disks.py: identical rays, only the float summation order differs
FLUX_TOL = 1e-4        # ... and on the source-normalised flux
SEED = 12345


@functools.lru_cache(maxsize=None)
def scene(name):
    """points, normals (read-only arrays), the number of rays and the source direction"""
    n, rays = (64, 4_000_000) if name == "e" else (32, 200_000)
    x0 = -(n - 1) / 2.0
    X, Y = np.meshgrid(x0 + np.arange(n), x0 + np.arange(n), indexing="ij")
    height = np.float32(0.3) if name in ("b", "c", "g") else np.float32(0.0)
    pts = np.stack([X.ravel(), Y.ravel(), np.full(n * n, height)], -1).astype(np.float32)
    nrm = np.tile(np.array([0, 0, 1], np.float32), (n * n, 1))
    direction = vr.TraceDirection.POS_Z
    if name in ("b", "c"):
        nrm = np.tile(np.array([-0.0, 0.0, 1.0], np.float32), (n * n, 1))
        assert nrm[0, 0].view(np.uint32) == 0x80000000
    if name == "c":
        k = 13 * n + 17  # an interior disk
        pts[k, 2] = np.nextafter(pts[k, 2], np.float32(1))
        assert int(pts[k, 2].view(np.uint32)) == int(height.view(np.uint32)) + 1
    if name == "d":
        v = np.array([0.1, 0.05, 1.0], np.float32)
        v = (v / np.sqrt((v * v).sum(dtype=np.float32))).astype(np.float32)
        nrm = np.tile(v, (n * n, 1))
    if name in ("f", "h"):
        nrm = np.tile(np.array([0, 0, -1], np.float32), (n * n, 1))
    if name == "h":
        direction = vr.TraceDirection.NEG_Z
    if name == "g":
        pts = np.ascontiguousarray(pts[:, [2, 0, 1]])  # the plane x = 0.3f
        nrm = np.tile(np.array([1, 0, 0], np.float32), (n * n, 1))
        direction = vr.TraceDirection.POS_X
    pts.setflags(write=False)
    nrm.setflags(write=False)
    return pts, nrm, rays, direction


def gpu_run(name, knob, monkeypatch, capfd):
    monkeypatch.setenv("VR_SMALL_SCENE", "0")
    monkeypatch.setenv("VR_PLANAR_DISKS", str(knob))
    monkeypatch.setenv("VR_PRINT_LAUNCHES", "1")
    pts, nrm, rays, direction = scene(name)
    t = vr.TraceDisk(3)
    t.setGeometry(pts, nrm, 1.0)
    t.setBoundaryConditions([BC.PERIODIC_BOUNDARY] * 3)
    t.setSourceDirection(direction)
    t.setParticleType(vr.DiffuseParticle(1.0, "flux"))
    t.setNumberOfRaysFixed(rays)
    t.setRngSeed(SEED)
    capfd.readouterr()
    t.apply()
    err = capfd.readouterr().err
    uni = re.search(r"\[vr\] uniform disks: scene (\d), VR_UNIFORM_DISKS (\d), launch (\d)", err)
    pla = re.search(r"\[vr\] planar disks: scene (\d), VR_PLANAR_DISKS (\d), launch (\d)", err)
    assert uni, "no uniform-disks line on stderr"
    assert pla, "no planar-disks line on stderr"
    assert err.index("[vr] uniform disks:") < err.index("[vr] planar disks:")
    info = t.getRayTraceInfo()
    return {"t": t, "f32": t.getLocalData().getVectorData(0).copy(), "f64": t.getFluxF64(), "mode": t.traceMode(),
            "info": {k: int(getattr(info, k)) for k in COUNTERS}, "uniform": tuple(int(v) for v in uni.groups()),
            "planar": tuple(int(v) for v in pla.groups())}


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    pts, nrm, rays, direction = scene(name)
    o = po.Oracle()
    o.set_disks(pts, nrm, 1.0, 3)
    o.set_boundary_conditions([po.PERIODIC] * 3)
    o.set_source_direction(int(direction))
    o.set_particle(po.DIFFUSE, 1.0)
    o.set_num_rays_fixed(rays)
    o.set_rng_seed(SEED)
    o.set_lazy_rng(True)
    o.apply(po.max_threads())
    return o, o.flux(), o.info()


def against_oracle(name, run):
    o, ref, oi = oracle_run(name)
    err = l2_rel(run["f32"], ref)
    print("  oracle L2", err, {k: oi[k] for k in ORACLE_COUNTERS})
    assert {k: run["info"][k] for k in ORACLE_COUNTERS} == {k: oi[k] for k in ORACLE_COUNTERS}, (run["info"], oi, err)
    assert err <= FLUX_ORDER_TOL, err
    assert l2_rel(run["t"].normalizeFlux(run["f32"]), o.normalize_flux(ref)) <= FLUX_TOL


@pytest.mark.parametrize("name", ["a", "b", "e", "f", "g", "h"])
def test_planar_variant_changes_no_result(name, monkeypatch, capfd):
    off = gpu_run(name, 0, monkeypatch, capfd)
    on = gpu_run(name, 1, monkeypatch, capfd)
    print(name, "modes", off["mode"], on["mode"], "uniform", off["uniform"], on["uniform"], "planar", off["planar"], on["planar"],
          on["info"])
    assert off["mode"] == 1 and on["mode"] == 1  # (the flat absorbing kernel; the variant is a kernel of that mode)
    assert off["uniform"] == (1, 1, 1) and on["uniform"] == (1, 1, 1)  # a kernel of the uniform family ran both times
    assert off["planar"] == (1, 0, 0)  # the knob forces the launch's flag false: the uniform-disk kernel
    assert on["planar"] == (1, 1, 1)
    assert on["info"] == off["info"], (off["info"], on["info"])
    if name == "f":  # (the disks face away from the source: met from behind, the ray goes on; nothing is credited)
        i = on["info"]
        assert i["geometryHits"] == 0 and i["totalRaysTraced"] - i["numRays"] - i["boundaryHits"] > 0, i
        assert on["f64"].sum() == 0 and off["f64"].sum() == 0
    else:
        assert on["info"]["geometryHits"] > 0
        assert on["f64"].sum() > 0
    assert np.array_equal(off["f64"], on["f64"])
    assert np.array_equal(off["f32"], on["f32"])
    against_oracle(name, on)


def test_one_centre_an_ulp_off_the_plane_clears_the_flag(monkeypatch, capfd):
    run = gpu_run("c", 1, monkeypatch, capfd)
    print("c: uniform", run["uniform"], "planar", run["planar"], run["info"])
    assert run["mode"] == 1
    assert run["uniform"] == (1, 1, 1)  # still uniform: the launch runs the uniform-disk kernel
    assert run["planar"] == (0, 1, 0)
    assert run["info"]["geometryHits"] > 0
    against_oracle("c", run)


def test_a_tilted_normal_is_not_planar(monkeypatch, capfd):
    run = gpu_run("d", 1, monkeypatch, capfd)
    print("d: uniform", run["uniform"], "planar", run["planar"], run["info"])
    assert run["mode"] == 1
    assert run["uniform"] == (1, 1, 1)
    assert run["planar"] == (0, 1, 0)
    assert run["info"]["geometryHits"] > 0
    against_oracle("d", run)
