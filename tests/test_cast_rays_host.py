"""The per-ray bookkeeping of castRays (viennaray_amd/csrc/vr_cast.hpp: what cast_rays_kernel folds every finished
segment into) on the host.  No GPU: tests/aux/cast_rays.cpp includes the header the kernel includes and runs a table of
segment sequences against the expected (prim, dist, boundaryHits, point) — the result codes, the tracer's boundary-hit
budget, IGNORE walls, a hit at exactly tmax — and 200 000 random chains for the tmax rule: a bounded cast is the unbounded
one with everything beyond tmax turned into a miss, and the path length never decreases.  The same program runs once more
built with AddressSanitizer and UndefinedBehaviorSanitizer, stand-alone."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "aux", "cast_rays.cpp")
INC = os.path.join(ROOT, "viennaray_amd", "csrc")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-I", INC]


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "\n0 failed checks" in out.stdout
    m = re.search(r"^(\d+) table cases, (\d+) random chains: (\d+) bounded results kept, (\d+) turned into a miss, "
                  r"(\d+) kept at exactly tmax$", out.stdout, flags=re.M)
    assert m, out.stdout
    cases, chains, kept, missed, exact = (int(v) for v in m.groups())
    assert cases >= 25 and chains >= 200_000
    # (the rule is about results that stay as much as about those that turn into a miss, and about the edge between them)
    assert kept >= chains // 10 and missed >= chains // 10 and exact >= chains // 20, (kept, missed, exact)
    return out


def test_cast_bookkeeping_table_and_tmax_rule(tmp_path):
    exe = str(tmp_path / "cast_rays")
    subprocess.check_call(["g++"] + FLAGS + [SRC, "-o", exe])
    _run(exe)


def test_cast_bookkeeping_under_sanitizers(tmp_path):
    """the same program with ASan and UBSan, run stand-alone (nothing is loaded into python)"""
    exe = str(tmp_path / "cast_rays_san")
    subprocess.check_call(["g++"] + FLAGS + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe])
    out = _run(exe)
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]


def test_entry_points_facade_and_python_methods_exist():
    """declared, exported and bound with the header's arity; tests/aux/facade_cast_rays.cpp compiles against the façade"""
    import inspect

    import viennaray_amd as vr
    from viennaray_amd import capi

    txt = open(os.path.join(ROOT, "include", "viennaray_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = vr.load()
    for name, arity in (("vr_cast_rays_device", 13), ("vr_cast_rays", 11)):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
        assert decl and len(decl.group(1).split(",")) == arity, name
        assert hasattr(L, name) and len(capi.SIGNATURES[name][1]) == arity, name
    for macro, value in (("VR_CAST_FOLLOW_BOUNDARIES", "1u"), ("VR_CAST_MISS", "(-1)"), ("VR_CAST_WALL", "(-2)")):
        assert re.search(r"#define\s+%s\s+%s" % (macro, re.escape(value)), code), macro
    assert (capi.VR_CAST_FOLLOW_BOUNDARIES, capi.VR_CAST_MISS, capi.VR_CAST_WALL) == (1, -1, -2)
    sig = inspect.signature(vr.Trace.castRays)
    assert list(sig.parameters) == ["self", "origins", "directions", "tmax", "followBoundaries", "tnear", "returnPoints",
                                    "returnBoundaryHits"]
    assert sig.parameters["tmax"].default == float("inf") and sig.parameters["followBoundaries"].default is True
    assert sig.parameters["tnear"].default == 1e-4
    assert list(inspect.signature(vr.Trace.occluded).parameters) == ["self", "origins", "targets"]
    hdr = open(os.path.join(ROOT, "include", "viennaray_amd", "viennaray.hpp")).read()
    for text in ("struct CastResult", "bool castRays(const std::vector<Vec3D<NumericType>> &origins", "bool castRaysDevice("):
        assert text in hdr, text
    flags = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", os.path.join(ROOT, "include", "viennaray_amd"),
             "-I", os.path.join(ROOT, "include")]
    p = subprocess.run(["g++", "-fsyntax-only"] + flags + [os.path.join(ROOT, "tests", "aux", "facade_cast_rays.cpp")],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]


def test_kernel_includes_the_header_the_host_program_tests():
    with open(os.path.join(INC, "vr_cast.hip")) as f:
        text = f.read()
    assert '#include "vr_cast.hpp"' in text
    for name in ("cast_begin", "cast_segment", "cast_ignored", "cast_finish"):
        assert re.search(r"\b%s\(" % name, text), name
