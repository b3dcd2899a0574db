"""The arithmetic of gatherFlux (viennaray_amd/csrc/vr_gather.hpp: what gather_samples_kernel computes a sample with) on
the host.  No GPU: tests/aux/gather.cpp includes the header the kernel includes and checks the outcome -> weight table for
every outcome, mode and dimension, q() and the final division at K = 1, 64, 65, 4096, the power guard, and the directions
of 10^5 samples per case (unit length within 2 ulp, the hemisphere, mean m.w = 2/3 and mean c = (n+1)/(n+2) within 5
sigma).  The same program runs once more built with AddressSanitizer and UndefinedBehaviorSanitizer, stand-alone."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "aux", "gather.cpp")
INC = os.path.join(ROOT, "viennaray_amd", "csrc")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-I", INC]


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "\n0 failed checks" in out.stdout
    m = re.search(r"^(\d+) checks$", out.stdout, flags=re.M)
    assert m and int(m.group(1)) >= 100_000, out.stdout
    return out


def test_gather_arithmetic(tmp_path):
    exe = str(tmp_path / "gather")
    subprocess.check_call(["g++"] + FLAGS + [SRC, "-o", exe])
    _run(exe)
    # the mode the GPU test compares vr_debug_gather_samples with: 64 lines of three hex floats
    out = subprocess.run([exe, "dirs", "7", "5", "3", "0", "0", "0x1p+0", "0", "3", "1", "2", "0", "1", "1"],
                         capture_output=True, text=True, timeout=60)
    rows = [[float.fromhex(v) for v in line.split()] for line in out.stdout.splitlines()]
    assert out.returncode == 0 and len(rows) == 64 and all(len(r) == 3 and r[2] > 0 for r in rows), out.stdout


def test_gather_arithmetic_under_sanitizers(tmp_path):
    """the same program with ASan and UBSan, run stand-alone (nothing is loaded into python)"""
    exe = str(tmp_path / "gather_san")
    subprocess.check_call(["g++"] + FLAGS + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe])
    out = _run(exe)
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]


def test_entry_points_facade_and_python_methods_exist():
    """declared, exported and bound with the header's arity; tests/aux/facade_gather_flux.cpp compiles against the façade"""
    import inspect

    import viennaray_amd as vr
    from viennaray_amd import capi

    txt = open(os.path.join(ROOT, "include", "viennaray_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = vr.load()
    for name, arity in (("vr_gather_flux_device", 9), ("vr_gather_flux", 8), ("vr_debug_gather_samples", 9)):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
        assert decl and len(decl.group(1).split(",")) == arity, name
        assert hasattr(L, name) and len(capi.SIGNATURES[name][1]) == arity, name
    for macro, value in (("VR_GATHER_NORMAL", "0u"), ("VR_GATHER_SOURCE", "1u"), ("VR_FLUX_FRAC_BITS", "40")):
        assert re.search(r"#define\s+%s\s+%s" % (macro, re.escape(value)), code), macro
    assert (capi.VR_GATHER_NORMAL, capi.VR_GATHER_SOURCE, capi.VR_FLUX_FRAC_BITS) == (0, 1, 40)
    assert (int(vr.GatherMode.NORMAL), int(vr.GatherMode.SOURCE)) == (0, 1)
    sig = inspect.signature(vr.Trace.gatherFlux)
    assert list(sig.parameters) == ["self", "samples", "cosinePower", "mode", "emission", "primFirst", "primCount", "numpy"]
    assert sig.parameters["cosinePower"].default == 1.0 and sig.parameters["mode"].default is vr.GatherMode.NORMAL
    assert sig.parameters["emission"].default is None and sig.parameters["primCount"].default is None
    hdr = open(os.path.join(ROOT, "include", "viennaray_amd", "viennaray.hpp")).read()
    for text in ("enum class GatherMode", "gatherFlux(unsigned samples, NumericType cosinePower = 1", "bool gatherFluxDevice("):
        assert text in hdr, text
    flags = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", os.path.join(ROOT, "include", "viennaray_amd"),
             "-I", os.path.join(ROOT, "include")]
    p = subprocess.run(["g++", "-fsyntax-only"] + flags + [os.path.join(ROOT, "tests", "aux", "facade_gather_flux.cpp")],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]


def test_kernel_includes_the_header_the_host_program_tests():
    with open(os.path.join(INC, "vr_gather.hip")) as f:
        text = f.read()
    assert '#include "vr_gather.hpp"' in text
    for name in ("gather_chunk_seed", "gather_direction", "gather_weight", "gather_q", "gather_result"):
        assert re.search(r"\b%s\(" % name, text), name
    # not a run-time model source: outside vr_trace.hip's closure
    mk = open(os.path.join(INC, "Makefile")).read()
    assert "vr_gather" not in re.findall(r"^MODEL_SRCS\s*:?=\s*(.*)$", mk, flags=re.M)[0]
