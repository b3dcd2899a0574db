"""Uniform disks (VR_UNIFORM_DISKS; pq_hit_packet UNIFORM, vr_packet_query.hpp): where every disk of the scene has one normal and
one radius, word for word, the 3-D absorbing flat-scene kernel computes the per-ray terms of its candidate tests once per
round and replaces the neighbour test's square root by a comparison.  That only removes repeated work: every case that
takes the variant runs once with VR_UNIFORM_DISKS=1 and once with =0, and the raw flux arrays are equal element for
element, as is every TraceInfo counter; each case also goes against the CPU oracle with the bounds of the existing plane
tests (tests/test_flat_absorbing_scalar.py, tests/test_aligned_bins.py: counters equal, flux L2-relative error <= 5e-6,
<= 1e-4 on the source-normalised flux).  The VR_PRINT_LAUNCHES line says whether the scene has the property and whether the
launch ran the variant.

The scenes: disks on a 32 x 32 lattice of pitch 1, periodic walls, 200 000 rays, seed 12345, DiffuseParticle of
sticking 1 — (a) normals (0, 0, 1): every product with the normal is exact; (b) every normal the normalised float vector
(0.1, 0.05, 1): the dot products round; (c) as (a) with one interior disk's n.x the smallest positive denormal: one word
differs, the flag must be clear; (e) a 64 x 64 lattice under 4 000 000 rays: rounds with full waves and several leaf
nodes per query.  (A disk with another RADIUS cannot be made: every setter of disks takes one radius for the cloud.)"""
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
FLUX_ORDER_TOL = 5e-6  # tests/test_flat_absorbing_scalar.py: identical rays, only the float summation order differs
FLUX_TOL = 1e-4        # ... and on the source-normalised flux
SEED = 12345


@functools.lru_cache(maxsize=None)
def scene(name):
    """points, normals (read-only arrays) and the number of rays"""
    n, rays = (64, 4_000_000) if name == "e" else (32, 200_000)
    x0 = -(n - 1) / 2.0
    X, Y = np.meshgrid(x0 + np.arange(n), x0 + np.arange(n), indexing="ij")
    pts = np.stack([X.ravel(), Y.ravel(), np.zeros(n * n)], -1).astype(np.float32)
    nrm = np.tile(np.array([0, 0, 1], np.float32), (n * n, 1))
    if name == "b":
        v = np.array([0.1, 0.05, 1.0], np.float32)
        v = (v / np.sqrt((v * v).sum(dtype=np.float32))).astype(np.float32)
        assert v[0] != 0 and v[1] != 0 and v[2] != 1
        nrm = np.tile(v, (n * n, 1))
    if name == "c":
        nrm[13 * n + 17, 0] = np.float32(1.401298464324817e-45)  # an interior disk; the smallest positive denormal
        assert nrm[13 * n + 17, 0].view(np.uint32) == 1
    pts.setflags(write=False)
    nrm.setflags(write=False)
    return pts, nrm, rays


def gpu_run(name, knob, monkeypatch, capfd):
    monkeypatch.setenv("VR_SMALL_SCENE", "0")
    monkeypatch.setenv("VR_UNIFORM_DISKS", str(knob))
    monkeypatch.setenv("VR_PRINT_LAUNCHES", "1")
    pts, nrm, rays = scene(name)
    t = vr.TraceDisk(3)
    t.setGeometry(pts, nrm, 1.0)
    t.setBoundaryConditions([BC.PERIODIC_BOUNDARY] * 3)
    t.setParticleType(vr.DiffuseParticle(1.0, "flux"))
    t.setNumberOfRaysFixed(rays)
    t.setRngSeed(SEED)
    capfd.readouterr()
    t.apply()
    line = re.search(r"\[vr\] uniform disks: scene (\d), VR_UNIFORM_DISKS (\d), launch (\d)", capfd.readouterr().err)
    assert line, "no uniform-disks line on stderr"
    info = t.getRayTraceInfo()
    return {"t": t, "f32": t.getLocalData().getVectorData(0).copy(), "f64": t.getFluxF64(), "mode": t.traceMode(),
            "info": {k: int(getattr(info, k)) for k in COUNTERS}, "scene": int(line.group(1)), "knob": int(line.group(2)),
            "launch": int(line.group(3))}


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    pts, nrm, rays = scene(name)
    o = po.Oracle()
    o.set_disks(pts, nrm, 1.0, 3)
    o.set_boundary_conditions([po.PERIODIC] * 3)
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


@pytest.mark.parametrize("name", ["a", "b", "e"])
def test_uniform_variant_changes_no_result(name, monkeypatch, capfd):
    off = gpu_run(name, 0, monkeypatch, capfd)
    on = gpu_run(name, 1, monkeypatch, capfd)
    print(name, "modes", off["mode"], on["mode"], "scene/knob/launch", [(r["scene"], r["knob"], r["launch"]) for r in (off, on)],
          on["info"])
    assert off["mode"] == 1 and on["mode"] == 1  # (the launch's mode stays MODE_ABSORB_FLAT: the variant is a kernel of that mode)
    assert (off["scene"], off["knob"], off["launch"]) == (1, 0, 0)  # the knob forces the launch's flag false
    assert (on["scene"], on["knob"], on["launch"]) == (1, 1, 1)
    assert on["info"] == off["info"], (off["info"], on["info"])
    assert on["info"]["geometryHits"] > 0 and on["f64"].sum() > 0
    assert np.array_equal(off["f64"], on["f64"])
    assert np.array_equal(off["f32"], on["f32"])
    against_oracle(name, on)


def test_one_differing_word_clears_the_flag(monkeypatch, capfd):
    run = gpu_run("c", 1, monkeypatch, capfd)
    print("c: scene/knob/launch", run["scene"], run["knob"], run["launch"], run["info"])
    assert run["mode"] == 1
    assert (run["scene"], run["knob"], run["launch"]) == (0, 1, 0)
    assert run["info"]["geometryHits"] > 0
    against_oracle("c", run)
