"""The arithmetic of solveRadiosity (viennaray_amd/csrc/vr_radiosity.hpp: the link table's index, a row of one iteration,
the reflectivity multiply, the residual and the stopping rule, as the kernels of vr_radiosity.hip compile them) on the
host.  No GPU: tests/aux/radiosity.cpp includes vr_radiosity.hpp and vr_gather.hpp only and checks two mutually facing
primitives by hand (F -> 2 monotonically, t and r_t as defined, maxIterations = 0), the residual's order over bit
patterns, the index beyond 2^32 entries, and the cut of an emission above wmax.  The program is built with
AddressSanitizer and UndefinedBehaviorSanitizer and run stand-alone; nothing is loaded into python."""
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "aux", "radiosity.cpp")
INC = os.path.join(ROOT, "viennaray_amd", "csrc")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-I", INC]


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "\n0 failed checks" in out.stdout
    m = re.search(r"^(\d+) checks$", out.stdout, flags=re.M)
    assert m and int(m.group(1)) >= 500_000, out.stdout
    return out


def test_radiosity_arithmetic_under_sanitizers(tmp_path):
    exe = str(tmp_path / "radiosity_san")
    subprocess.check_call(["g++"] + FLAGS + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe])
    out = _run(exe)
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]


def test_host_program_takes_the_two_headers_alone():
    text = open(SRC).read()
    assert sorted(re.findall(r'#include "([^"]+)"', text)) == ["vr_gather.hpp", "vr_radiosity.hpp"]
    hpp = open(os.path.join(INC, "vr_radiosity.hpp")).read()
    assert re.findall(r'#include "([^"]+)"', hpp) == ["vr_gather.hpp"]


def test_kernels_use_the_header_the_host_program_tests():
    it = open(os.path.join(INC, "vr_radiosity.hip")).read()
    assert '#include "vr_radiosity.hpp"' in it
    for name in ("radiosity_link_index", "radiosity_link_q", "radiosity_row_result", "radiosity_emission",
                 "radiosity_residual_bits", "radiosity_stops", "radiosity_rho_ok"):
        assert re.search(r"\b%s\(" % name, it), name
    # nothing of a walk in the iteration's unit: no trace kernel header, no RNG, no stack
    for word in ("vr_trace_kernel.hpp", "vr_rng.hpp", "vr_walk.hpp", "pair_walk", "mt_step", "stackS"):
        assert word not in it, word
    # one text for what a sample is: the recording is the gather's kernel under a compile-time flag, not a second loop
    g = open(os.path.join(INC, "vr_gather.hip")).read()
    assert '#include "vr_radiosity.hpp"' in g and "radiosity_link_index(" in g
    assert len(re.findall(r"__global__[^;{]*\bgather_samples_kernel\b", g)) == 1
    assert len(re.findall(r"pair_walk_lanes<", g)) == 1
    for geo, d in ((0, 2), (0, 3), (1, 2), (1, 3)):
        for rec in ("true", "false"):
            assert "gather_samples_kernel<%d, %d, %s>" % (geo, d, rec) in g
    mk = open(os.path.join(INC, "Makefile")).read()
    assert "vr_radiosity.hip" in mk and "vr_radiosity_solve.cpp" in mk
    assert "vr_radiosity" not in re.findall(r"^MODEL_SRCS\s*:?=\s*(.*)$", mk, flags=re.M)[0]


def test_entry_points_facade_and_python_methods_exist():
    """declared, exported and bound with the header's arity; tests/aux/facade_radiosity.cpp compiles against the façade"""
    import viennaray_amd as vr
    from viennaray_amd import capi

    txt = open(os.path.join(ROOT, "include", "viennaray_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = vr.load()
    for name, arity in (("vr_radiosity_link_bytes", 2), ("vr_radiosity_links_device", 4), ("vr_radiosity_resident", 3),
                        ("vr_radiosity_solve_device", 9), ("vr_radiosity_solve", 8), ("vr_radiosity_direct_device", 3),
                        ("vr_debug_radiosity_links", 5), ("vr_debug_radiosity_time_iterations", 5),
                        ("vr_radiosity_free_links", 1)):
        decl = re.search(r"\b(?:int|uint64_t)\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
        assert decl and len(decl.group(1).split(",")) == arity, name
        assert hasattr(L, name) and len(capi.SIGNATURES[name][1]) == arity, name
    sig = inspect.signature(vr.Trace.solveRadiosity)
    assert list(sig.parameters) == ["self", "samples", "sticking", "reflectivity", "cosinePower", "tolerance", "maxIterations",
                                    "returnInfo"]
    assert sig.parameters["cosinePower"].default == 1.0 and sig.parameters["tolerance"].default == 1e-4
    assert sig.parameters["maxIterations"].default == 1000 and sig.parameters["returnInfo"].default is False
    for method in ("radiosityLinks", "radiosityLinkBytes", "debugRadiosityLinks", "freeRadiosityLinks"):
        assert callable(getattr(vr.Trace, method)), method
    hdr = open(os.path.join(ROOT, "include", "viennaray_amd", "viennaray.hpp")).read()
    for text in ("solveRadiosity(unsigned samples, NumericType sticking", "bool solveRadiosityDevice(", "bool radiosityLinks("):
        assert text in hdr, text
    flags = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", os.path.join(ROOT, "include", "viennaray_amd"),
             "-I", os.path.join(ROOT, "include")]
    p = subprocess.run(["g++", "-fsyntax-only"] + flags + [os.path.join(ROOT, "tests", "aux", "facade_radiosity.cpp")],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
