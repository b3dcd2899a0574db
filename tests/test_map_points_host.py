"""Per-primitive values at the caller's points (vr_map_to_points*): what holds without a GPU — the three entry points are
declared, exported and bound, the façade and the Python methods exist, and the brute-force reference
(tests/map_points_ref.py) answers hand-made cases as the definition says."""
import inspect
import os
import re
import subprocess

import numpy as np

import viennaray_amd as vr
from viennaray_amd import capi

import map_points_ref as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACADE_FLAGS = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include",
                "-I", os.path.join(ROOT, "include", "viennaray_amd"), "-I", os.path.join(ROOT, "include")]
ARITY = {"vr_map_to_points_device": 10, "vr_map_to_points": 8, "vr_get_flux_at_points_device": 11}


def test_the_three_symbols_are_declared_exported_and_bound():
    txt = open(os.path.join(ROOT, "include", "viennaray_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = vr.load()
    for name, arity in ARITY.items():
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
        assert decl, f"{name} is not declared"
        assert len(decl.group(1).split(",")) == arity, name
        assert hasattr(L, name), f"{name} is not exported"
        assert len(capi.SIGNATURES[name][1]) == arity, name
    # the definition is in the header: range, weight, fallback, what is not applied
    for phrase in ("in range iff d_ij < R", "(1 - d_ij / R)", "lowest original id", "periodicity is NOT applied", "NaN"):
        assert phrase in txt, phrase


def test_cpp_facade_declares_the_map():
    """tests/aux/facade_map_points.cpp compiles against the façade"""
    hdr = open(os.path.join(ROOT, "include", "viennaray_amd", "viennaray.hpp")).read()
    for name in ("bool mapToPointsDevice(", "bool getFluxAtPointsDevice(", "mapToPoints(const std::vector<NumericType> &values"):
        assert name in hdr, name
    src = os.path.join(ROOT, "tests", "aux", "facade_map_points.cpp")
    p = subprocess.run(["g++", "-fsyntax-only"] + FACADE_FLAGS + [src], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]


def test_python_methods_exist():
    sig = inspect.signature(vr.Trace.mapToPoints)
    assert list(sig.parameters) == ["self", "values", "points", "normals", "radius"]
    assert sig.parameters["normals"].default is None and sig.parameters["radius"].default is None
    sig = inspect.signature(vr.Trace.getFluxAtPoints)
    assert list(sig.parameters) == ["self", "points", "normals", "radius", "dataIdx", "norm", "numNeighbors"]
    assert sig.parameters["dataIdx"].default == 0 and sig.parameters["numNeighbors"].default == 0
    for cls in (vr.TraceDisk, vr.TraceTriangle):
        assert callable(cls.mapToPoints) and callable(cls.getFluxAtPoints)


def test_the_sort_threshold_is_a_knob_of_the_table():
    src = open(os.path.join(ROOT, "viennaray_amd", "csrc", "vr_knobs.cpp")).read()
    assert 'getenv("VR_MAP_SORT_MIN")' in src
    mk = open(os.path.join(ROOT, "viennaray_amd", "csrc", "Makefile")).read()
    assert "vr_map.hip" in mk


# ---- the reference on hand-made cases --------------------------------------------------------------------------------
UP = np.array([[0.0, 0.0, 1.0]])


def test_reference_one_primitive():
    for R in (0.0, 0.5, 10.0):
        r = mp.reference([3.5], [[1, 2, 3]], UP, [[0, 0, 0], [1, 2, 3], [9, 9, 9]], None, R)
        # ((w * f) / w in float64: within a rounding of f where the mean applies, f itself where it does not)
        assert np.allclose(r["out"], 3.5, rtol=1e-15, atol=0) and np.array_equal(r["jstar"], [0, 0, 0])
        assert np.array_equal(r["out"][r["sum_w"] == 0], np.full(int((r["sum_w"] == 0).sum()), 3.5))
        assert np.isinf(r["gap"]).all()


def test_reference_query_on_a_centre_returns_its_value_exactly():
    c = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float32)
    f = np.array([0.1, 0.7, 0.9], dtype=np.float32)
    r = mp.reference(f, c, np.repeat(UP, 3, 0), c, None, 0.5)  # only the centre itself is within 0.5
    assert np.array_equal(r["out"], f.astype(np.float64)) and np.array_equal(r["K"], [1, 1, 1])
    assert np.array_equal(r["sum_w"], [1.0, 1.0, 1.0]) and not r["ambiguous"].any()
    r0 = mp.reference(f, c, np.repeat(UP, 3, 0), c, None, 0.0)
    assert np.array_equal(r0["out"], f.astype(np.float64)) and np.array_equal(r0["K"], [0, 0, 0])
    assert np.array_equal(r0["jstar"], [0, 1, 2])


def test_reference_two_centres_at_a_quarter_and_three_quarters():
    R = 2.0
    c = [[-R / 4, 0, 0], [3 * R / 4, 0, 0]]
    r = mp.reference([10.0, 20.0], c, np.repeat(UP, 2, 0), [[0, 0, 0]], None, R)
    assert r["K"][0] == 2 and r["sum_w"][0] == 1.0
    assert r["out"][0] == 0.75 * 10.0 + 0.25 * 20.0
    assert r["jstar"][0] == 0 and r["gap"][0] == 8.0  # (9/16 - 1/16) / (1/16)
    assert np.array_equal(mp.tolerance(r, [10.0, 20.0]), [(2 + 8) * 2.0 ** -23 * 20.0])


def test_reference_normal_gate_removes_one_of_two_neighbours():
    c = [[-0.5, 0, 0], [0.5, 0, 0]]
    nj = [[0, 0, 1], [0, 0, -1]]
    r = mp.reference([1.0, 5.0], c, nj, [[0.1, 0, 0]], [[0, 0, 3.0]], 2.0)  # (normalised: any length)
    assert r["K"][0] == 2 and r["out"][0] == 1.0 and r["jstar"][0] == 1  # the mean takes 0, the nearest would be 1
    assert abs(r["sum_w"][0] - (1 - 0.6 / 2.0)) < 1e-15
    # every normal facing away: the nearest centre's value, normals or not
    r = mp.reference([1.0, 5.0], c, [[0, 0, -1], [0, 0, -1]], [[0.1, 0, 0]], [[0, 0, 1.0]], 2.0)
    assert r["sum_w"][0] == 0.0 and r["out"][0] == 5.0 and mp.tolerance(r, [1.0, 5.0])[0] == 0.0
    # a tie goes to the lowest id
    r = mp.reference([1.0, 5.0], c, nj, [[0, 3, 0]], None, 0.0)
    assert r["jstar"][0] == 0 and r["gap"][0] == 0.0 and r["ambiguous_nearest"][0] and not r["ambiguous"][0]


def test_reference_two_dimensions_ignore_z():
    c = [[0, 0, 50.0], [1, 0, -7.0]]
    nj = [[0, 1, 9.0], [0, 1, -9.0]]
    p3 = [[0.25, 0, 123.0]]
    p2 = [[0.25, 0]]
    a = mp.reference([2.0, 4.0], c, nj, p3, [[0, 2.0, 5.0]], 1.0, D=2)
    b = mp.reference([2.0, 4.0], c, nj, p2, [[0, 1.0]], 1.0, D=2)
    assert a["out"][0] == b["out"][0] == (0.75 * 2.0 + 0.25 * 4.0) and a["K"][0] == 2
    far = mp.reference([2.0, 4.0], c, nj, p3, None, 1.0, D=3)
    assert far["K"][0] == 0 and far["out"][0] == 2.0


def test_reference_flags_the_ambiguous():
    c = [[1.0, 0, 0]]
    r = mp.reference([1.0], c, UP, [[0, 0, 0]], None, 1.0 + 5e-6)
    assert r["ambiguous"][0]
    r = mp.reference([1.0], c, UP, [[0, 0, 0]], None, 1.04)  # in range, weight 0.038
    assert r["ambiguous"][0] and 0 < r["sum_w"][0] < 0.05
    r = mp.reference([1.0], c, UP, [[0, 0, 0], [np.nan, 0, 0], [0, np.inf, 0]], None, 2.0)
    assert not r["ambiguous"].any() and np.isnan(r["out"][1:]).all() and r["out"][0] == 1.0


def test_centroids_are_float32_by_the_stated_formula():
    v = np.array([[0.1, 0.2, 0.3], [1.1, 0.7, 0.3], [0.4, 2.2, 0.3]], dtype=np.float32)
    c = mp.triangle_centroids(v, [[0, 1, 2]])
    third = np.float32(1.0 / 3.0)
    assert c.dtype == np.float32
    assert c[0, 0] == np.float32(np.float32(np.float32(v[0, 0] + v[1, 0]) + v[2, 0]) * third)
