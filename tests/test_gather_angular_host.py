"""The arithmetic of the angular gather (viennaray_amd/csrc/vr_gather.hpp: gather_law, gather_law_norm, gather_law_g, the
validity rules, gather_path_weight_laws) on the host.  No GPU: tests/aux/gather_angular.cpp includes vr_gather.hpp alone,
the text the kernels compile; it runs once plain and once under AddressSanitizer and UndefinedBehaviorSanitizer,
stand-alone.  numpy float32 in the header's operation order reproduces the look-up bit for bit — the rule
tests/test_gather_angular.py replays is the device's — and the normalisation agrees with an independent quadrature
(tests/angular_forms.py).  Entry points, ctypes signatures, Python signatures, the façade and the launch texts of
vr_gather.hip are checked as their neighbours check theirs."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import angular_forms as af

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "aux", "gather_angular.cpp")
INC = os.path.join(ROOT, "viennaray_amd", "csrc")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-I", INC]


def np_law(table, x):
    """gather_law in numpy float32, one operation at a time in vr_gather.hpp's order; table [M], x [...]"""
    t = np.asarray(table, dtype=np.float32)
    M = len(t)
    x = np.asarray(x, dtype=np.float32)
    xc = np.fmin(np.fmax(x, np.float32(0)), np.float32(1))  # (fmax / fmin: a NaN x gives the other argument, 0)
    xs = (xc * np.float32(M - 1)).astype(np.float32)
    k = np.minimum(xs.astype(np.int32), M - 2)
    f = (xs - k.astype(np.float32)).astype(np.float32)
    d = (t[k + 1] - t[k]).astype(np.float32)
    return (t[k] + (f * d).astype(np.float32)).astype(np.float32)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gather_angular") / "gather_angular")
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


def test_look_up_normalisation_rules_and_weights(program):
    _run(program)


def test_arithmetic_under_sanitizers(tmp_path):
    """the same program with ASan and UBSan, run stand-alone (nothing is loaded into python)"""
    exe = str(tmp_path / "gather_angular_san")
    subprocess.check_call(["g++"] + FLAGS + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe])
    out = _run(exe)
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]


def test_host_program_takes_the_header_alone():
    text = open(SRC).read()
    assert re.findall(r'#include "([^"]+)"', text) == ["vr_gather.hpp"]
    hpp = open(os.path.join(INC, "vr_gather.hpp")).read()
    for name in ("gather_law", "gather_law_norm", "gather_law_g", "gather_law_entry_ok", "gather_path_weight_laws"):
        assert re.search(r"\b%s\(" % name, hpp), name
    start = hpp.index("float gather_law(")
    assert "VR_GATHER_NO_CONTRACT" in hpp[start - 200:start + 300]  # contraction off, like gather_moments


def _hex(v):
    return "nan" if np.isnan(v) else float(v).hex()


def test_numpy_reproduces_the_look_up_bit_for_bit(program):
    """10^4 random (table, M, x): M = 2, 3 and 256 among them; x = 0, 1, -0.0, just below 1, NaN and outside [0, 1]"""
    rng = np.random.default_rng(23)
    special = [0.0, 1.0, -0.0, float(np.nextafter(np.float32(1), np.float32(0))), float("nan"), -0.25, 1.5, float("inf"),
               float("-inf"), 1e-30, 0.5]
    rows, want = [], []
    for r in range(10_000):
        M = (2, 3, 256, 255, 33)[r % 5] if r % 2 == 0 else int(rng.integers(2, 257))
        kind = r % 4
        table = rng.random(M).astype(np.float32) * np.float32((1.0, 3.0, 1e-3, 1e4)[kind])
        if r % 17 == 0:
            table[:] = table[0]
        x = np.float32(special[(r // 5) % len(special)]) if r % 3 == 0 else np.float32(rng.random())
        if r % 29 == 0:  # on a node
            x = np.float32(int(rng.integers(0, M))) / np.float32(M - 1)
        rows.append("%d %s %s" % (M, _hex(x), " ".join(_hex(v) for v in table)))
        want.append(np_law(table, x))
    out = subprocess.run([program, "law"], input="\n".join(rows) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and len(out.stdout.splitlines()) == len(rows), out.stderr[-2000:]
    got = np.array([float.fromhex(line) for line in out.stdout.splitlines()], dtype=np.float32)
    want = np.array(want, dtype=np.float32)
    assert not np.isnan(got).any()
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert len(bad) == 0, [(rows[i][:60], float(got[i]), float(want[i])) for i in bad[:5]]


def _norm_rows(program, rows):
    text = "\n".join("%d %d %s" % (D, len(t), " ".join(float(v).hex() for v in t)) for D, t in rows) + "\n"
    out = subprocess.run([program, "norm"], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and len(out.stdout.splitlines()) == len(rows), out.stderr[-2000:]
    return [(float.fromhex(line.split()[0]), np.float32(float.fromhex(line.split()[1]))) for line in out.stdout.splitlines()]


def test_normalisation_against_an_independent_quadrature(program):
    """tables sampled from c^(n - 1), n = 1, 2, 8, both dimensions, several M: Z within 1e-12 relative of Gauss-Legendre
    over each linear segment (10^4 nodes or more in all), g_L = (float)(pi / Z), (float)(2 / Z)"""
    rows, powers = [], []
    for D in (2, 3):
        for n in (1, 2, 8):
            for M in (2, 3, 33, 256):
                c = np.linspace(0.0, 1.0, M)
                rows.append((D, (c ** (n - 1)).astype(np.float32)))
                powers.append(n)
    got = _norm_rows(program, rows)
    for (D, t), (Z, gL) in zip(rows, got):
        per = -(-10_000 // (len(t) - 1))  # nodes per segment: at least 10^4 in all
        ref = af.norm3(t, per) if D == 3 else af.norm2(t, max(per, 40))
        assert abs(Z / ref - 1.0) <= 1e-12, (D, len(t), Z, ref)
        assert gL == np.float32((np.pi if D == 3 else 2.0) / Z)
    # c^(n - 1) itself: the interpolant of M = 256 nodes is close to the law, Z to pi 2 / (n + 1) and to C_n
    import math
    for (D, t), (Z, _), n in zip(rows, got, powers):
        if len(t) == 256:
            exact = 2 * math.pi / (n + 1) if D == 3 else math.sqrt(math.pi) * math.gamma((n + 1) / 2) / math.gamma(n / 2 + 1)
            assert abs(Z / exact - 1.0) < 1e-3, (D, n, Z, exact)


def test_all_ones_normalise_to_exactly_one(program):
    rows = [(D, np.ones(M, np.float32)) for D in (2, 3) for M in (2, 3, 7, 256)]
    for (D, t), (Z, gL) in zip(rows, _norm_rows(program, rows)):
        assert gL.view(np.uint32) == np.float32(1.0).view(np.uint32), (D, len(t), Z, gL)


def test_closed_forms_are_converged():
    """the quadratures the GPU tests compare against, at the node counts they use: twice the nodes change nothing beyond
    1e-6; the limits they must reduce to"""
    import closed_forms as cf
    c = np.linspace(0.0, 1.0, 33)
    L = (c ** 2 * (1 + c) / 2).astype(np.float32)
    x = np.array([-4.5 - 1 / 6, -2.0, 0.0, 1 / 3, 4.5 + 1 / 6])
    z = np.array([-1 / 3, -5 - 2 / 3, -10 + 1 / 3])
    for fn, args, n in ((af.source_bottom, (L, x), 128), (af.source_bottom_2d, (L, x), 256), (af.yield_wall, ([0.5, 3.0], z), 32),
                        (af.reflectivity_bottom, ([1.0, 0.2], 0.8, x), 16)):
        _, diff = af.converged(fn, *args, n=n)
        assert diff <= 1e-6, (fn.__name__, diff)
    assert np.abs(af.yield_wall([1.0, 1.0], z, 32) - af.yield_wall_unit(z)).max() < 1e-12
    assert np.abs(af.reflectivity_bottom([1.0, 1.0], 0.8, x, 16) - cf.specular_bottom(cf.W, cf.DEPTH, 0.2, x)).max() < 1e-9
    assert np.abs(af.source_bottom(np.ones(5), x, 64) - cf.power_cosine_bottom(cf.W, cf.DEPTH, 1.0, x)).max() < 1e-9
    assert abs(af.norm3(np.ones(9)) / np.pi - 1) < 1e-14 and abs(af.norm2(np.ones(9)) / 2 - 1) < 1e-14


def test_entry_points_facade_and_python_methods_exist():
    import viennaray_amd as vr
    from viennaray_amd import capi

    txt = open(os.path.join(ROOT, "include", "viennaray_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = vr.load()
    for name, arity in (("vr_gather_angular_device", 8), ("vr_gather_angular", 7), ("vr_gather_angular_sums_device", 11),
                        ("vr_gather_angular_sums", 10), ("vr_gather_angular_adaptive_device", 14), ("vr_gather_angular_adaptive", 13),
                        ("vr_debug_gather_angular_path", 13)):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
        assert decl and len(decl.group(1).split(",")) == arity, name
        assert "const vr_gather_spec *spec, const vr_gather_laws *laws" in decl.group(1), name
        assert hasattr(L, name) and len(capi.SIGNATURES[name][1]) == arity, name
    # the old arities and the spec stay as they were
    for name, arity in (("vr_gather_paths_device", 11), ("vr_gather_paths", 10), ("vr_debug_gather_path", 16),
                        ("vr_gather_sums_device", 10), ("vr_gather_sums", 9), ("vr_gather_adaptive_device", 13),
                        ("vr_gather_adaptive", 12)):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
        assert decl and len(decl.group(1).split(",")) == arity and len(capi.SIGNATURES[name][1]) == arity, name
    assert ctypes.sizeof(capi.GatherSpecPOD) == 48
    for field in ("sourceLaw", "sourceCount", "reflectivityLaw", "reflectivityCount", "yieldLaw", "yieldCount"):
        assert re.search(r"typedef struct vr_gather_laws \{[^}]*\b%s;" % field, code), field
    assert [f for f, _ in capi.GatherLawsPOD._fields_] == ["sourceLaw", "sourceCount", "reflectivityLaw", "reflectivityCount",
                                                           "yieldLaw", "yieldCount"]
    assert ctypes.sizeof(capi.GatherLawsPOD) == 48 and capi.GatherLawsPOD.yieldLaw.offset == 32
    sig = inspect.signature(vr.Trace.gatherAngular)
    assert list(sig.parameters)[:12] == ["self", "samples", "sourceLaw", "reflectivityLaw", "yieldLaw", "sticking", "reflectivity",
                                         "reflection", "maxBounces", "primFirst", "primCount", "numpy"]
    assert "stickingLaw" in sig.parameters and sig.parameters["maxBounces"].default == 64
    assert sig.parameters["reflection"].default is vr.GatherReflection.SPECULAR
    sig = inspect.signature(vr.Trace.gatherAngularAdaptive)
    assert list(sig.parameters)[:5] == ["self", "target", "sourceLaw", "reflectivityLaw", "yieldLaw"]
    assert (sig.parameters["minSamples"].default, sig.parameters["maxSamples"].default) == (64, 4096)
    assert list(inspect.signature(vr.Trace.gatherAngularSums).parameters)[:4] == ["self", "chunkFirst", "chunks", "budget"]
    assert "laws" in inspect.signature(vr.Trace.debugGatherAngularPath).parameters
    # the pinned signatures of the neighbours
    assert list(inspect.signature(vr.Trace.gatherPaths).parameters) == ["self", "samples", "sticking", "reflectivity", "reflection",
                                                                        "maxBounces", "cosinePower", "primFirst", "primCount", "numpy"]
    hdr = open(os.path.join(ROOT, "include", "viennaray_amd", "viennaray.hpp")).read()
    for text in ("gatherAngular(unsigned samples, const GatherLaws &laws", "bool gatherAngularDevice(", "gatherAngularAdaptive(",
                 "bool gatherAngularSums(", "bool debugGatherAngularPath("):
        assert text in hdr, text
    flags = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", os.path.join(ROOT, "include", "viennaray_amd"),
             "-I", os.path.join(ROOT, "include")]
    p = subprocess.run(["g++", "-fsyntax-only"] + flags + [os.path.join(ROOT, "tests", "aux", "facade_gather_angular.cpp")],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]


def test_kernel_keeps_its_launch_texts_and_gains_the_law_instantiations():
    with open(os.path.join(INC, "vr_gather.hip")) as f:
        text = f.read()
    assert len(re.findall(r"__global__[^;{]*\bgather_samples_kernel\b", text)) == 1
    assert len(re.findall(r"pair_walk_lanes<", text)) == 1
    assert re.search(r"template <int GEO, int D, bool REC, int PATH = 0, int STAT = 0>", text)
    for geo in (0, 1):
        for d in (2, 3):
            # the 24 old launches, word for word
            for tail in ("false>)", "true>)", "false, 1>)", "false, 2>)", "false, 0, 1>)", "false, 1, 1>)"):
                assert "gather_samples_kernel<%d, %d, %s" % (geo, d, tail) in text, (geo, d, tail)
            # the laws: a further value of PATH, fixed K and the sums
            assert "gather_samples_kernel<%d, %d, false, 3>)" % (geo, d) in text
            assert "gather_samples_kernel<%d, %d, false, 3, 1>)" % (geo, d) in text
            assert "gather_samples_kernel<%d, %d, true, 3" % (geo, d) not in text
    assert "gather_samples_kernel<" in text and not re.search(r"gather_samples_kernel<\d, \d, false, 4", text)  # no fourth family
    assert "__shared__ float lawBuf[3 * GATHER_LAW_MAX]" in text  # the laws are staged in LDS
    for name in ("gather_path_weight_laws", "gather_path_throughput_law"):
        assert re.search(r"\b%s\(" % name, text), name
    mk = open(os.path.join(INC, "Makefile")).read()
    assert "vr_gather_angular.cpp" in mk
