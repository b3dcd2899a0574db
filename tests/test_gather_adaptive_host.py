"""The arithmetic of the gather to a target error (viennaray_amd/csrc/vr_gather.hpp: gather_q2, gather_stderr2,
gather_converged) on the host.  No GPU: tests/aux/gather_adaptive.cpp includes vr_gather.hpp alone, the text the kernels
compile, and checks the squared weight against 128-bit integers, the overflow bound for every power-of-two budget and the
standard error against long double; it runs once plain and once under AddressSanitizer and UndefinedBehaviorSanitizer,
stand-alone.  numpy float64 in the header's operation order reproduces gather_stderr2 bit for bit: the rule
tests/test_gather_adaptive.py replays is the device's.  Entry points, ctypes signatures, Python signatures, the façade and
the launch texts of vr_gather.hip are checked as their neighbours check theirs."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "aux", "gather_adaptive.cpp")
INC = os.path.join(ROOT, "viennaray_amd", "csrc")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-I", INC]


def np_moments(S1, S2, K):
    """(m1, se2) in numpy float64, one operation at a time in vr_gather.hpp's order"""
    k = np.asarray(K, dtype=np.float64)
    m1 = np.asarray(S1, dtype=np.int64).astype(np.float64) * np.float64(2.0 ** -40) / k
    m2 = np.asarray(S2, dtype=np.int64).astype(np.float64) * np.float64(2.0 ** -28) / k
    v = m2 - m1 * m1
    v = np.where(v > 0, v, 0.0)
    return m1, v / (k - 1.0)


def np_converged(S1, S2, K, rel, absolute=0.0):
    m1, se2 = np_moments(S1, S2, K)
    tol = np.maximum(np.float64(np.float32(rel)) * m1, np.float64(np.float32(absolute)))
    return se2 <= tol * tol


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gather_adaptive") / "gather_adaptive")
    subprocess.check_call(["g++"] + FLAGS + [SRC, "-o", exe])
    return exe


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[-2000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "\n0 failed checks" in out.stdout
    m = re.search(r"^(\d+) checks$", out.stdout, flags=re.M)
    assert m and int(m.group(1)) >= 400_000, out.stdout[-2000:]
    return out


def test_second_sum_and_standard_error_arithmetic(program):
    _run(program)


def test_arithmetic_under_sanitizers(tmp_path):
    """the same program with ASan and UBSan, run stand-alone (nothing is loaded into python)"""
    exe = str(tmp_path / "gather_adaptive_san")
    subprocess.check_call(["g++"] + FLAGS + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe])
    out = _run(exe)
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]


def test_host_program_takes_the_header_alone():
    text = open(SRC).read()
    assert re.findall(r'#include "([^"]+)"', text) == ["vr_gather.hpp"]
    hpp = open(os.path.join(INC, "vr_gather.hpp")).read()
    assert "GATHER_SQ_FRAC_BITS = 28" in hpp and "static_assert" in hpp
    for name in ("gather_q2", "gather_stderr2", "gather_converged"):
        assert re.search(r"\b%s\(" % name, hpp), name
    assert "fp contract(off)" in hpp


def test_numpy_reproduces_the_standard_error_bit_for_bit(program):
    """some thousand random (S1, S2, K): sums of K samples of random weights quantised as the header quantises them, and
    raw random sums with S2 far from S1^2 / K, the v <= 0 side included"""
    rng = np.random.default_rng(11)
    rows = []
    for _ in range(3000):
        K = 64 << int(rng.integers(0, 7))
        w = rng.random(K) * rng.choice([1.0, 4.5, 0.01]) * (rng.random(K) < rng.random())
        q1 = np.floor(w.astype(np.float32).astype(np.float64) * 2.0 ** 40 + 0.5).astype(np.int64)
        q2 = np.floor(w.astype(np.float32).astype(np.float64) ** 2 * 2.0 ** 28 + 0.5).astype(np.int64)
        rows.append((int(q1.sum()), int(q2.sum()), K))
    for _ in range(3000):
        K = 64 * int(rng.integers(1, 65))
        rows.append((int(rng.integers(0, 1 << 52)), int(rng.integers(0, 1 << 40)), K))
    text = "\n".join("%d %d %d" % r for r in rows) + "\n"
    out = subprocess.run([program, "se2"], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and len(out.stdout.splitlines()) == len(rows)
    got = np.array([float.fromhex(line.split()[0]) for line in out.stdout.splitlines()], dtype=np.float64)
    verdict = np.array([int(line.split()[1]) for line in out.stdout.splitlines()], dtype=bool)
    S1, S2, K = (np.array(c, dtype=np.int64) for c in zip(*rows))
    _, se2 = np_moments(S1, S2, K)
    assert (se2.view(np.uint64) == got.view(np.uint64)).all()
    assert (se2 == 0).sum() > 100 and (se2 > 0).sum() > 1000  # both sides of the v > 0 test were met
    assert (np_converged(S1, S2, K, 0.05) == verdict).all()
    assert verdict.sum() > 100 and (~verdict).sum() > 100


def test_entry_points_facade_and_python_methods_exist():
    import viennaray_amd as vr
    from viennaray_amd import capi

    txt = open(os.path.join(ROOT, "include", "viennaray_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = vr.load()
    for name, arity in (("vr_gather_sums_device", 10), ("vr_gather_sums", 9), ("vr_gather_adaptive_device", 13),
                        ("vr_gather_adaptive", 12)):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
        assert decl and len(decl.group(1).split(",")) == arity, name
        assert hasattr(L, name) and len(capi.SIGNATURES[name][1]) == arity, name
    for field in ("cosinePower", "mode", "emission", "paths", "reflection", "maxBounces", "reflectivity", "reflectivityScalar"):
        assert re.search(r"typedef struct vr_gather_spec \{[^}]*\b%s;" % field, code), field
    assert [f for f, _ in capi.GatherSpecPOD._fields_] == ["cosinePower", "mode", "emission", "paths", "reflection", "maxBounces",
                                                           "reflectivity", "reflectivityScalar"]
    import ctypes
    assert ctypes.sizeof(capi.GatherSpecPOD) == 48 and capi.GatherSpecPOD.reflectivity.offset == 32
    assert [f for f, _ in capi.GatherAdaptiveInfoPOD._fields_] == ["rounds", "unconverged", "totalSamples"]
    assert ctypes.sizeof(capi.GatherAdaptiveInfoPOD) == 16
    sig = inspect.signature(vr.Trace.gatherFluxAdaptive)
    assert list(sig.parameters)[:11] == ["self", "target", "minSamples", "maxSamples", "absTarget", "cosinePower", "mode", "emission",
                                         "primFirst", "primCount", "returnInfo"]
    assert (sig.parameters["minSamples"].default, sig.parameters["maxSamples"].default) == (64, 4096)
    assert sig.parameters["absTarget"].default == 0.0 and sig.parameters["returnInfo"].default is False
    sig = inspect.signature(vr.Trace.gatherPathsAdaptive)
    assert list(sig.parameters)[:13] == ["self", "target", "sticking", "reflectivity", "reflection", "maxBounces", "minSamples",
                                         "maxSamples", "absTarget", "cosinePower", "primFirst", "primCount", "returnInfo"]
    assert sig.parameters["maxBounces"].default == 64 and sig.parameters["reflection"].default is vr.GatherReflection.SPECULAR
    for method in ("gatherFluxSums", "gatherPathsSums"):
        assert callable(getattr(vr.Trace, method)), method
    # the fixed-K calls keep their signatures
    assert list(inspect.signature(vr.Trace.gatherFlux).parameters) == ["self", "samples", "cosinePower", "mode", "emission",
                                                                       "primFirst", "primCount", "numpy"]
    hdr = open(os.path.join(ROOT, "include", "viennaray_amd", "viennaray.hpp")).read()
    for text in ("gatherFluxAdaptive(NumericType relTarget, unsigned minSamples", "gatherPathsAdaptive(NumericType relTarget, "
                 "NumericType sticking", "bool gatherAdaptiveDevice(", "bool gatherSums("):
        assert text in hdr, text
    flags = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", os.path.join(ROOT, "include", "viennaray_amd"),
             "-I", os.path.join(ROOT, "include")]
    p = subprocess.run(["g++", "-fsyntax-only"] + flags + [os.path.join(ROOT, "tests", "aux", "facade_gather_adaptive.cpp")],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]


def test_kernel_keeps_its_launch_texts_and_gains_the_stat_instantiations():
    with open(os.path.join(INC, "vr_gather.hip")) as f:
        text = f.read()
    assert len(re.findall(r"__global__[^;{]*\bgather_samples_kernel\b", text)) == 1
    assert len(re.findall(r"pair_walk_lanes<", text)) == 1
    assert re.search(r"template <int GEO, int D, bool REC, int PATH = 0, int STAT = 0>", text)
    for geo in (0, 1):
        for d in (2, 3):
            # the old launches, word for word
            assert "gather_samples_kernel<%d, %d, false>)" % (geo, d) in text
            assert "gather_samples_kernel<%d, %d, true>)" % (geo, d) in text
            assert "gather_samples_kernel<%d, %d, false, 1>)" % (geo, d) in text
            assert "gather_samples_kernel<%d, %d, false, 2>)" % (geo, d) in text
            # the sums: a fifth argument, without the recording, for samples and for paths
            assert "gather_samples_kernel<%d, %d, false, 0, 1>)" % (geo, d) in text
            assert "gather_samples_kernel<%d, %d, false, 1, 1>)" % (geo, d) in text
            assert "gather_samples_kernel<%d, %d, true, 0, 1>" % (geo, d) not in text
    for name in ("gather_q2", "gather_converged", "gather_stderr2", "gather_result"):
        assert re.search(r"\b%s\(" % name, text), name
    assert "gather_decide_kernel" in text and "atomicAdd(d.next" not in text  # the next list is built without an atomic append
    start = text.index("void gather_decide_kernel")
    decide = text[start:text.index("debug_gather_samples_kernel", start)]
    assert "atomic" not in decide and "ballot64(" in decide
    mk = open(os.path.join(INC, "Makefile")).read()
    assert "vr_gather_adaptive.cpp" in mk
