"""The arithmetic of gatherPaths (viennaray_amd/csrc/vr_gather.hpp: the counter draw of a diffuse vertex, the throughput
update, the end -> weight rule; vr_math.hpp: reflect_specular) on the host.  No GPU: tests/aux/gather_paths.cpp includes
the headers the kernel includes.  The counter draw is a pure function of (seed, primitive, sample, bounce), differs
between neighbours, lies in [0, 1) and has the moments of a uniform within 5 sigma; reflect_specular agrees with numpy
float32 in the header's operation order; T = 1 leaves the gather's weight bit for bit and every other end weighs 0.  The
same program runs once more built with AddressSanitizer and UndefinedBehaviorSanitizer, stand-alone."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "aux", "gather_paths.cpp")
INC = os.path.join(ROOT, "viennaray_amd", "csrc")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-I", INC]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gather_paths") / "gather_paths")
    subprocess.check_call(["g++"] + FLAGS + [SRC, "-o", exe])
    return exe


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[-2000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "\n0 failed checks" in out.stdout
    m = re.search(r"^(\d+) checks$", out.stdout, flags=re.M)
    assert m and int(m.group(1)) >= 100_000, out.stdout[-2000:]
    return out


def test_path_arithmetic(program):
    _run(program)


def test_counter_draw_has_the_moments_of_a_uniform(program):
    """2^16 draws: the mean of r1 and of r1 r2 within 5 sigma of 1/2 and 1/4, sigma from the uniform's own variances
    (1/12, and E[r1^2] E[r2^2] - 1/16 = 7/144 for independent uniforms); the 24-bit grid shifts the mean by 2^-25"""
    for seed in (7, 12345):
        out = subprocess.run([program, "stats", str(seed)], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr
        m1, m12, lo, hi, n = out.stdout.split()
        n = int(n)
        assert n == 1 << 16
        print("seed %d: mean r1 %.6f (%.2f sigma), mean r1 r2 %.6f (%.2f sigma)"
              % (seed, float(m1), abs(float(m1) - 0.5) / math.sqrt(1 / 12 / n), float(m12),
                 abs(float(m12) - 0.25) / math.sqrt(7 / 144 / n)))
        assert abs(float(m1) - 0.5) <= 5 * math.sqrt(1 / 12 / n) + 2.0 ** -25
        assert abs(float(m12) - 0.25) <= 5 * math.sqrt(7 / 144 / n) + 2.0 ** -25
        assert 0.0 <= float(lo) and float(hi) < 1.0


def test_draws_mode_is_reproducible_and_keyed_by_all_four_inputs(program):
    def draws(*a):
        out = subprocess.run([program, "draws"] + [str(v) for v in a], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0
        return out.stdout

    base = draws(7, 5, 3, 8)
    assert base == draws(7, 5, 3, 8) and len(base.splitlines()) == 8
    assert base.splitlines()[:4] == draws(7, 5, 3, 4).splitlines()  # (a bounce's draw does not depend on how many follow)
    for other in ((8, 5, 3, 8), (7, 6, 3, 8), (7, 5, 4, 8)):
        assert not set(base.splitlines()) & set(draws(*other).splitlines()), other


def test_reflect_specular_agrees_with_numpy_float32(program):
    rng = np.random.default_rng(3)
    d = rng.normal(size=(200, 3)).astype(np.float32)
    n = rng.normal(size=(200, 3)).astype(np.float32)
    n /= np.linalg.norm(n, axis=1, keepdims=True).astype(np.float32)
    text = "\n".join(" ".join(float(v).hex() for v in list(a) + list(b)) for a, b in zip(d, n))
    out = subprocess.run([program, "reflect"], input=text, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0
    got = np.array([[float.fromhex(v) for v in line.split()] for line in out.stdout.splitlines()], dtype=np.float32)
    inv = -d
    f = np.float32(2) * ((n[:, 0] * inv[:, 0] + n[:, 1] * inv[:, 1]) + n[:, 2] * inv[:, 2])
    ref = f[:, None] * n - inv
    assert ref.dtype == np.float32 and got.shape == ref.shape
    assert (got.view(np.uint32) == ref.view(np.uint32)).all()


def test_path_arithmetic_under_sanitizers(tmp_path):
    """the same program with ASan and UBSan, run stand-alone (nothing is loaded into python)"""
    exe = str(tmp_path / "gather_paths_san")
    subprocess.check_call(["g++"] + FLAGS + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe])
    out = _run(exe)
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]


def test_entry_points_facade_and_python_methods_exist():
    import inspect

    import viennaray_amd as vr
    from viennaray_amd import capi

    txt = open(os.path.join(ROOT, "include", "viennaray_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = vr.load()
    for name, arity in (("vr_gather_paths_device", 11), ("vr_gather_paths", 10), ("vr_debug_gather_path", 16)):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
        assert decl and len(decl.group(1).split(",")) == arity, name
        assert hasattr(L, name) and len(capi.SIGNATURES[name][1]) == arity, name
    for macro, value in (("VR_GATHER_REFLECT_SPECULAR", "0u"), ("VR_GATHER_REFLECT_DIFFUSE", "1u"), ("VR_GATHER_MAX_BOUNCES", "65535u"),
                         ("VR_GATHER_END_BOUNCES", "5"), ("VR_GATHER_END_ABSORBED", "6")):
        assert re.search(r"#define\s+%s\s+%s\b" % (macro, re.escape(value)), code), macro
    assert (int(vr.GatherReflection.SPECULAR), int(vr.GatherReflection.DIFFUSE)) == (0, 1)
    assert (capi.VR_GATHER_END_BOUNCES, capi.VR_GATHER_END_ABSORBED, capi.VR_GATHER_MAX_BOUNCES) == (5, 6, 65535)
    sig = inspect.signature(vr.Trace.gatherPaths)
    assert list(sig.parameters) == ["self", "samples", "sticking", "reflectivity", "reflection", "maxBounces", "cosinePower",
                                    "primFirst", "primCount", "numpy"]
    assert sig.parameters["maxBounces"].default == 64 and sig.parameters["reflection"].default is vr.GatherReflection.SPECULAR
    assert hasattr(vr.Trace, "debugGatherPath")
    hdr = open(os.path.join(ROOT, "include", "viennaray_amd", "viennaray.hpp")).read()
    for text in ("enum class GatherReflection", "gatherPaths(unsigned samples, NumericType sticking", "bool gatherPathsDevice("):
        assert text in hdr, text
    flags = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", os.path.join(ROOT, "include", "viennaray_amd"),
             "-I", os.path.join(ROOT, "include")]
    p = subprocess.run(["g++", "-fsyntax-only"] + flags + [os.path.join(ROOT, "tests", "aux", "facade_gather_paths.cpp")],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]


def test_kernel_steps_through_the_header_the_host_program_tests():
    with open(os.path.join(INC, "vr_gather.hip")) as f:
        text = f.read()
    for name in ("gather_path_diffuse", "gather_path_throughput", "gather_path_weight", "reflect_specular", "project_dir<D>"):
        assert re.search(r"\b%s\(" % re.escape(name), text), name
    # the instantiations of the gather and of the link recording are launched as before; the paths are a fourth argument
    for geo in (0, 1):
        for d in (2, 3):
            assert "gather_samples_kernel<%d, %d, false>)" % (geo, d) in text
            assert "gather_samples_kernel<%d, %d, true>)" % (geo, d) in text
            assert "gather_samples_kernel<%d, %d, false, 1>)" % (geo, d) in text
