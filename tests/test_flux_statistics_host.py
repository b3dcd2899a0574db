"""Flux statistics without a GPU: the C++ façade's members compile, link and do not crash; the Python entry points fail
with the library's message; and the calibration the GPU test (tests/test_flux_statistics.py, test 7) leans on — the
per-credit estimator against the run-to-run scatter — holds on the oracle's own event sums."""
import os
import subprocess

import numpy as np
import pytest

import viennaray_amd as vr
from viennaray_amd import capi
from oracle import pyoracle as po
from helpers import ROOT, trench_mesh

FACADE_FLAGS = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include",
                "-I", os.path.join(ROOT, "include", "viennaray_amd"), "-I", os.path.join(ROOT, "include")]
FACADE_SRC = os.path.join(ROOT, "tests", "aux", "facade_flux_statistics.cpp")
NEW_SYMBOLS = ("vr_set_flux_statistics", "vr_get_hit_counts", "vr_get_flux_sum_squares", "vr_get_flux_error",
               "vr_get_flux_error_device")


def _build_facade(tmp_path):
    exe = tmp_path / "facade_flux_statistics"
    lib = os.path.join(ROOT, "viennaray_amd")
    subprocess.check_call(["g++", "-O1"] + FACADE_FLAGS + [FACADE_SRC, "-o", str(exe), "-L", lib, "-lviennaray_amd",
                                                          "-L", "/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib,
                                                          "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_facade_flux_statistics_builds_and_runs(tmp_path):
    """tests/aux/facade_flux_statistics.cpp calls every new façade member; without a device it must end cleanly, with
    one it checks the members against each other"""
    exe = _build_facade(tmp_path)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "facade flux statistics ok" in out.stdout, out.stdout + out.stderr
    if not vr.device_available():
        assert "(no device)" in out.stdout


def test_entry_points_are_declared_exported_and_typed():
    L = vr.load()
    header = open(os.path.join(ROOT, "include", "viennaray_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert name in header and hasattr(L, name) and name in capi.SIGNATURES
    # a NULL context is refused, not dereferenced
    assert L.vr_set_flux_statistics(None, 1) != 0
    out = np.zeros(4, dtype=np.uint64)
    import ctypes as C
    assert L.vr_get_hit_counts(None, 0, C.c_void_p(out.ctypes.data), 4) != 0
    assert L.vr_get_flux_error(None, 0, 0, C.c_void_p(out.ctypes.data), 4) != 0


def test_python_members_exist_and_fail_with_the_library_message_without_a_gpu():
    for name in ("setCalculateFluxError", "getHitCounts", "getFluxSumSquares", "getFluxRelativeError", "getFluxAbsoluteError",
                 "getFluxErrorTensor", "getFluxErrorDevice", "raysForRelativeError", "numAccumulatorPlanes"):
        assert callable(getattr(vr.TraceDisk, name)) and callable(getattr(vr.TraceTriangle, name))
    if vr.device_available():
        t = vr.TraceDisk(3)
        with pytest.raises(vr.VrError, match="statistics are off"):
            t.getHitCounts()
        t.setCalculateFluxError(True)
        with pytest.raises(vr.VrError, match="no result"):
            t.getFluxRelativeError()
    else:
        with pytest.raises(vr.VrError) as e:   # (the tracer itself cannot exist: the library says why)
            vr.TraceDisk(3).setCalculateFluxError(True)
        assert str(e.value)


def test_distributed_statistics_from_accumulators():
    """the layout and the formula of the multi-GPU driver's summary: labels, then sum of squares, then hits, per particle"""
    from viennaray_amd.distributed import flux_statistics_from_accumulators
    two40 = 1 << 40
    n = 3
    # particle 0: one label; particle 1: two labels.  Primitive 2 is never reached.
    acc = np.array([[4 * two40, two40 // 2, 0], [16 * two40 // 4, two40 // 4, 0], [4, 1, 0],
                    [two40, two40, 0], [7, 7, 7], [two40, two40, 0], [1, 1, 0]], dtype=np.int64).reshape(-1)
    hits, rel = flux_statistics_from_accumulators(acc, n, [1, 2], 100)
    assert hits[0].tolist() == [4, 1, 0] and hits[1].tolist() == [1, 1, 0]
    s1, sq = 4.0, 4.0
    assert rel[0][0] == np.float32(np.sqrt(sq - s1 * s1 / 100) / s1) and np.isposinf(rel[0][2]) and np.isposinf(rel[1][2])
    assert rel[0][1] == np.float32(np.sqrt(0.25 - 0.25 / 100) / 0.5) and rel[0].dtype == np.float32


def test_estimator_matches_the_scatter_of_the_oracle():
    """trenchMesh.dat, DiffuseParticle(0.3), 200 000 rays, seed 77, run numbers 0 .. 23, from the oracle's event log:
    pooled over the triangles with non-zero mean flux, sqrt(sum emp^2 / sum pred^2) — emp the sample standard deviation
    (ddof 1) of the raw flux over the runs, pred^2 the mean over the runs of sumsq - S1^2 / N — is 0.996 (measured); the
    sampling error of the pooled ratio over 12 800 triangles x 23 degrees of freedom is about 0.2 %."""
    gd, v, tri = trench_mesh()
    n, rays, runs = len(tri), 200_000, 24
    o = po.Oracle()
    o.set_triangles(v, tri, gd, 3)
    o.set_particle(po.DIFFUSE, 0.3)
    o.set_num_rays_fixed(rays)
    o.set_rng_seed(77)
    o.set_lazy_rng(True)
    o.set_event_capacity(50_000_000)
    s1s, var = [], []
    for run in range(runs):
        o.set_run_number(run)
        o.apply(1)
        ev = o.events()
        sel = ev["kind"] == 3
        prim, w = ev["prim"][sel].astype(np.int64), ev["weight"][sel].astype(np.float64)
        s1 = np.bincount(prim, weights=w, minlength=n)
        sq = np.bincount(prim, weights=w * w, minlength=n)
        s1s.append(s1)
        var.append(np.maximum(sq - s1 * s1 / rays, 0.0))
    s1s, var = np.array(s1s), np.array(var)
    pool = s1s.mean(axis=0) != 0
    assert pool.mean() >= 0.99
    emp = s1s.std(axis=0, ddof=1)[pool]
    pred = np.sqrt(var.mean(axis=0))[pool]
    ratio = float(np.sqrt((emp ** 2).sum() / (pred ** 2).sum()))
    print(f"oracle: pooled emp / pred = {ratio:.4f} over {int(pool.sum())} of {n} triangles")
    assert 0.99 <= ratio <= 1.01, ratio
