"""The tile buckets of a lattice-lanes launch (VR_TILE_BUCKETS; vr_tile_buckets.hpp, vr_lattice_tiles.hpp): the generator
files the simple rays — wall-free, their plane point valid — by lattice tile with one global atomic per (chunk, tile), a
tile kernel finishes them against the tile's disks in LDS, and every other ray goes through the record stream's overflow
region and the lattice-lanes kernel as before.  Same rays, the acceptance and crediting arithmetic of trace_kernel on the same record bits,
integer sums: every case runs once with VR_TILE_BUCKETS=0 and once with =1 (VR_SMALL_SCENE=0 both times) and the raw float32
and float64 flux, every TraceInfo counter and the two statistics planes are equal element for element.  One case per group
also goes against the CPU oracle with the bounds of tests/test_gpu_parity.py::compare as tests/test_lattice_lanes.py states
them (counters equal, flux L2-relative error <= 5e-6: identical rays, only the float summation order differs; <= 1e-4 on
the source-normalised flux).  The VR_PRINT_LAUNCHES line "[vr] tile buckets:" says whether the launch ran the pipeline and
which share of its rays the lattice-lanes kernel traced instead.

The source plane sits at the top of the cloud's padded bounding box, h = 0.8 grid cells above the disks, and cannot be
moved, so the share of rays that cross a wall is set by the lattice's size: about perimeter x h / area for a cosine source.
The wall cases use a 16 x 12 lattice (56 x 0.8 / 192: more than a fifth of the rays); the 70 x 50 plane has about 6 %.

The index arithmetic of the tiles is checked on the host by tests/aux/lattice_tiles.cpp (no GPU)."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import viennaray_amd as vr
from viennaray_amd import BoundaryCondition as BC, TraceDirection as TD
from oracle import pyoracle as po
from helpers import l2_rel
from test_aligned_bins import lattice, rippled_plane

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = ("numRays", "totalRaysTraced", "nonGeometryHits", "geometryHits", "particleHits", "boundaryHits", "reflections",
            "raysTerminated", "rngFullStates")
ORACLE_COUNTERS = ("totalRaysTraced", "nonGeometryHits", "geometryHits", "boundaryHits", "reflections", "raysTerminated")
FLUX_ORDER_TOL = 5e-6  # tests/test_lattice_lanes.py
FLUX_TOL = 1e-4        # ... and on the source-normalised flux
SEED, RAYS = 4711, 200_000
PER, REF = BC.PERIODIC_BOUNDARY, BC.REFLECTIVE_BOUNDARY
TILE_LINE = (r"\[vr\] tile buckets: VR_TILE_BUCKETS (\d), launch (\d), tiles (\d+) \((\d+) x (\d+) of (\d+) cells a side\), "
             r"slices (\d+), other rays (\S+), handed on (\S+), particle")
KERNEL_LINE = r"\[vr\] kernel: traceMode (\d+), kernel mode (\d+), particle 0"


@functools.lru_cache(maxsize=None)
def scene(name):
    """points, normals (read-only), gridDelta"""
    if name == "plane70x50":
        pts, nrm = lattice(70, 50)
    elif name == "holes70x50":  # 5 % of the disks removed, seeded: rays through the holes miss the geometry
        pts, nrm = lattice(70, 50)
        keep = np.random.default_rng(20260117).random(len(pts)) >= 0.05
        assert 0.03 * len(pts) < (~keep).sum() < 0.07 * len(pts)
        pts, nrm = pts[keep], nrm[keep]
    elif name == "walls16x12":
        pts, nrm = lattice(16, 12)
    else:
        assert name == "ripple40"
        pts, nrm = rippled_plane(40)
    pts, nrm = np.ascontiguousarray(pts), np.ascontiguousarray(nrm)
    pts.setflags(write=False)
    nrm.setflags(write=False)
    return pts, nrm, 1.0


def tracer(name, bc, direction, sticking, rays, stats):
    pts, nrm, gd = scene(name)
    t = vr.TraceDisk(3)
    t.setGeometry(pts, nrm, gd)
    t.setBoundaryConditions([bc] * 3)
    t.setSourceDirection(direction)
    t.setParticleType(vr.DiffuseParticle(sticking, "flux"))
    t.setNumberOfRaysFixed(rays)
    t.setRngSeed(SEED)
    if stats:
        t.setCalculateFluxError(True)
    return t


def result(t, err, stats):
    line, kern = re.search(TILE_LINE, err), re.search(KERNEL_LINE, err)
    assert line, "no tile-bucket line on stderr"
    assert kern, "no kernel line on stderr"
    info = t.getRayTraceInfo()
    out = {"t": t, "f32": t.getLocalData().getVectorData(0).copy(), "f64": t.getFluxF64(), "mode": t.traceMode(),
           "kernel": int(kern.group(2)), "info": {k: int(getattr(info, k)) for k in COUNTERS}, "knob": int(line.group(1)),
           "launch": int(line.group(2)), "tiles": int(line.group(3)), "cells": int(line.group(6)),
           "other": float(line.group(8)), "handed": float(line.group(9))}
    if stats:
        out["hits"], out["sumsq"] = t.getHitCounts().copy(), t.getFluxSumSquares().copy()
    return out


def gpu_run(name, knob, monkeypatch, capfd, bc=PER, direction=TD.POS_Z, sticking=1.0, rays=RAYS, stats=False, env=(), ray_range=None):
    for k in ("VR_TILE_SHIFT", "VR_TILE_CAP", "VR_BATCH_RAYS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("VR_SMALL_SCENE", "0")
    monkeypatch.setenv("VR_TILE_BUCKETS", str(knob))
    monkeypatch.setenv("VR_PRINT_LAUNCHES", "1")
    for k, v in env:
        monkeypatch.setenv(k, v)
    t = tracer(name, bc, direction, sticking, rays, stats)
    if ray_range:
        t.setRayRange(*ray_range)
    capfd.readouterr()
    t.apply()
    return result(t, capfd.readouterr().err, stats)


@functools.lru_cache(maxsize=None)
def oracle_run(name, bc, direction, rays):
    pts, nrm, gd = scene(name)
    o = po.Oracle()
    o.set_disks(pts, nrm, gd, 3)
    o.set_boundary_conditions([int(bc)] * 3)
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
    err = l2_rel(run["f32"], ref) if ref.any() else float(np.abs(run["f32"]).max())
    print("  oracle L2", err, {k: oi[k] for k in ORACLE_COUNTERS})
    assert err <= FLUX_ORDER_TOL, err
    if ref.any():
        assert l2_rel(run["t"].normalizeFlux(run["f32"]), o.normalize_flux(ref)) <= FLUX_TOL


def same_bits(off, on, stats=False):
    assert (off["knob"], on["knob"]) == (0, 1)
    assert off["launch"] == 0
    assert (on["mode"], on["kernel"]) == (off["mode"], off["kernel"])
    assert on["info"] == off["info"], (off["info"], on["info"])
    assert np.array_equal(off["f64"], on["f64"])
    assert np.array_equal(off["f32"].view(np.uint32), on["f32"].view(np.uint32))
    if stats:
        assert np.array_equal(off["hits"], on["hits"]) and np.array_equal(off["sumsq"], on["sumsq"])


# (case id: scene, walls, source side, rays, environment, against the oracle, the tile's cells a side, tiles)
PLANE_CASES = {
    "plane-default": ("plane70x50", PER, TD.POS_Z, RAYS, (), True, 64, 2 * 1),
    "plane-tiles16": ("plane70x50", PER, TD.POS_Z, RAYS, (("VR_TILE_SHIFT", "4"),), False, 16, 5 * 4),   # 71 / 16, 51 / 16: partly filled tiles
    "plane-tiles4-reflective": ("plane70x50", REF, TD.POS_Z, RAYS, (("VR_TILE_SHIFT", "2"),), False, 4, 18 * 13),
    "holes-tiles16": ("holes70x50", PER, TD.POS_Z, RAYS, (("VR_TILE_SHIFT", "4"),), True, 16, 5 * 4),
    "holes-default": ("holes70x50", REF, TD.POS_Z, RAYS, (), False, 64, 2 * 1),
    "short-batch": ("plane70x50", PER, TD.POS_Z, 1_000, (("VR_TILE_SHIFT", "4"),), False, 16, 5 * 4),   # less than one chunk of 1024
    "odd-count": ("plane70x50", PER, TD.POS_Z, 200_003, (("VR_TILE_SHIFT", "4"),), True, 16, 5 * 4),    # no multiple of a block or a chunk
    "three-batches": ("plane70x50", PER, TD.POS_Z, RAYS, (("VR_TILE_SHIFT", "4"), ("VR_BATCH_RAYS", "70000")), False, 16, 5 * 4),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(PLANE_CASES))
def test_tile_buckets_change_no_result(case, monkeypatch, capfd):
    name, bc, direction, rays, env, oracle, cells, tiles = PLANE_CASES[case]
    off = gpu_run(name, 0, monkeypatch, capfd, bc, direction, rays=rays, stats=True, env=env)
    on = gpu_run(name, 1, monkeypatch, capfd, bc, direction, rays=rays, stats=True, env=env)
    print(case, "launch", on["launch"], "tiles", on["tiles"], "of", on["cells"], "other rays", on["other"], "handed on", on["handed"], on["info"])
    assert (off["mode"], off["kernel"]) == (1, 12)
    assert on["launch"] == 1 and on["cells"] == cells and on["tiles"] == tiles
    same_bits(off, on, stats=True)
    assert on["info"]["geometryHits"] > 0 and on["f64"].sum() > 0
    assert 0.0 < on["other"] < 1.0  # some rays cross a wall, most do not
    if name == "holes70x50":
        assert on["info"]["nonGeometryHits"] > 0 and on["handed"] > 0.0  # rays through the holes: handed on by the tile kernel
    if oracle:
        against_oracle(on, oracle_run(name, bc, direction, rays))


@pytest.mark.gpu
@pytest.mark.parametrize("bc", [PER, REF], ids=["periodic", "reflective"])
@pytest.mark.parametrize("direction", [TD.POS_Z, TD.NEG_Z], ids=["above", "below"])
def test_walls_and_either_source_side(bc, direction, monkeypatch, capfd):
    env = (("VR_TILE_SHIFT", "2"),)
    off = gpu_run("walls16x12", 0, monkeypatch, capfd, bc, direction, env=env)
    on = gpu_run("walls16x12", 1, monkeypatch, capfd, bc, direction, env=env)
    print("walls", int(bc), int(direction), "other rays", on["other"], "handed on", on["handed"], on["info"])
    same_bits(off, on)
    assert on["info"]["boundaryHits"] > 0
    if direction == TD.NEG_Z:
        # from below every hit is a back-face hit, which the tile kernel could not end: prepare keeps the parent's path
        assert on["launch"] == 0 and on["tiles"] == 0 and (on["mode"], on["kernel"]) == (1, 12)
    else:
        assert on["launch"] == 1 and on["cells"] == 4 and on["tiles"] == 5 * 4
        assert on["other"] > 0.0  # the rays that cross a wall are the lattice-lanes kernel's
    against_oracle(on, oracle_run("walls16x12", bc, direction, RAYS))


@pytest.mark.gpu
def test_ray_range_halves_sum_to_the_whole(monkeypatch, capfd):
    env = (("VR_TILE_SHIFT", "4"),)
    whole = gpu_run("plane70x50", 1, monkeypatch, capfd, REF, env=env)
    first, second = 100_037, RAYS - 100_037  # (a split inside a chunk and inside a wave)
    a = gpu_run("plane70x50", 1, monkeypatch, capfd, REF, env=env, ray_range=(0, first))
    b = gpu_run("plane70x50", 1, monkeypatch, capfd, REF, env=env, ray_range=(first, second))
    assert a["launch"] == 1 and b["launch"] == 1
    assert np.array_equal(a["f64"] + b["f64"], whole["f64"])  # (counts of unit weights: exact in float64)
    for k in COUNTERS[1:]:
        assert a["info"][k] + b["info"][k] == whole["info"][k], k
    off = gpu_run("plane70x50", 0, monkeypatch, capfd, REF, env=env, ray_range=(first, second))
    same_bits(off, b)


@pytest.mark.gpu
def test_a_small_bucket_spills_to_the_overflow_region(monkeypatch, capfd):
    roomy = gpu_run("plane70x50", 1, monkeypatch, capfd, env=(("VR_TILE_SHIFT", "4"),))
    off = gpu_run("plane70x50", 0, monkeypatch, capfd, env=(("VR_TILE_SHIFT", "4"),))
    tight = gpu_run("plane70x50", 1, monkeypatch, capfd, env=(("VR_TILE_SHIFT", "4"), ("VR_TILE_CAP", "1000")))
    print("spill: other rays", roomy["other"], "->", tight["other"])
    # 20 buckets of 1000 slots hold at most a tenth of the 200 000 rays
    assert tight["launch"] == 1 and tight["other"] >= 0.9 > roomy["other"]
    same_bits(off, tight)
    same_bits(off, roomy)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["rippled", "sticking0.1"])
def test_ineligible_launches_keep_the_parents_path(case, monkeypatch, capfd):
    name, sticking = ("ripple40", 1.0) if case == "rippled" else ("plane70x50", 0.1)
    off = gpu_run(name, 0, monkeypatch, capfd, sticking=sticking)
    on = gpu_run(name, 1, monkeypatch, capfd, sticking=sticking)
    print(case, "traceMode", on["mode"], "kernel", on["kernel"])
    assert on["launch"] == 0 and on["tiles"] == 0
    assert (on["mode"], on["kernel"]) == (off["mode"], off["kernel"]) == ((5, 5) if case == "rippled" else (3, 3))
    assert on["info"] == off["info"]
    assert np.array_equal(off["f64"], on["f64"])


def test_tile_index_arithmetic_on_the_host(tmp_path):
    """tests/aux/lattice_tiles.cpp: tiles, halo and slots against brute force; a simple ray's four corners inside tile + halo"""
    exe = str(tmp_path / "lattice_tiles")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Werror", "-I",
                           os.path.join(ROOT, "viennaray_amd", "csrc"), os.path.join(ROOT, "tests", "aux", "lattice_tiles.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    assert "lattice_tiles: ok" in out.stdout
