"""The adaptive species gather on the host (vr_gather_species_adaptive*: every species of a primitive to its own target
error along one set of traced paths).  No GPU: tests/aux/gather_species_adaptive.cpp includes vr_gather.hpp alone — the
per-species step and the per-entry verdict the kernels compile — and runs once plain and once under AddressSanitizer and
UndefinedBehaviorSanitizer, stand-alone.  Entry points, ctypes signatures, the Python signature, the façade and the kernel
file's shape are checked as the neighbours check theirs."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "aux", "gather_species_adaptive.cpp")
INC = os.path.join(ROOT, "viennaray_amd", "csrc")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-I", INC]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gather_species_adaptive") / "gather_species_adaptive")
    subprocess.check_call(["g++"] + FLAGS + [SRC, "-o", exe])
    return exe


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[-2000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "\n0 failed checks" in out.stdout
    m = re.search(r"^(\d+) checks$", out.stdout, flags=re.M)
    assert m and int(m.group(1)) >= 50_000, out.stdout[-2000:]
    # at least 10^4 (primitive, species) streams, and they reach what the masks are for
    m = re.search(r"^(\d+) streams, (\d+) trials whose species stop at different K, (\d+) unconverged, (\d+) rounds started from a "
                  r"partial mask$", out.stdout, flags=re.M)
    assert m and int(m.group(1)) >= 10_000 and all(int(m.group(k)) > 100 for k in (2, 3, 4)), out.stdout[-2000:]
    return out


def test_every_species_stops_where_its_own_call_stops(program):
    _run(program)


def test_rounds_under_sanitizers(tmp_path):
    """the same program with ASan and UBSan, run stand-alone (nothing is loaded into python)"""
    exe = str(tmp_path / "gather_species_adaptive_san")
    subprocess.check_call(["g++"] + FLAGS + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe])
    out = _run(exe)
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]


def test_host_program_takes_the_header_alone():
    text = open(SRC).read()
    assert re.findall(r'#include "([^"]+)"', text) == ["vr_gather.hpp"]
    assert re.search(r"\bint main\(", text)
    for name in ("gather_species_decide(", "gather_species_absorb<NS>(", "gather_species_reflect<NS>(", "gather_converged(",
                 "gather_result(", "gather_stderr2("):
        assert name in text, name
    hpp = open(os.path.join(INC, "vr_gather.hpp")).read()
    assert re.search(r"VR_GATHER_FN unsigned gather_species_decide\(", hpp)  # host/device, returning the next mask


def test_entry_points_facade_and_python_method_exist():
    import viennaray_amd as vr
    from viennaray_amd import capi

    txt = open(os.path.join(ROOT, "include", "viennaray_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = vr.load()
    for name, arity in (("vr_gather_species_adaptive_device", 15), ("vr_gather_species_adaptive", 14)):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
        assert decl and len(decl.group(1).split(",")) == arity, name
        assert "const vr_gather_spec *specs, const vr_gather_laws *laws, uint32_t numSpecies" in decl.group(1), name
        assert "const float *relTargets, const float *absTargets" in decl.group(1), name
        assert "vr_gather_species_adaptive_info *info" in decl.group(1), name
        assert hasattr(L, name) and len(capi.SIGNATURES[name][1]) == arity, name
    assert re.search(r"typedef struct vr_gather_species_adaptive_info \{\s*uint32_t rounds;"
                     r"\s*uint32_t unconverged\[VR_GATHER_MAX_SPECIES\];\s*uint64_t totalSamples\[VR_GATHER_MAX_SPECIES\];"
                     r"\s*uint64_t walkedSamples;\s*\}", code)
    assert "An adaptive species call is not offered" not in txt
    # rounds, 4 x uint32, (padding), 4 x uint64, uint64
    assert ctypes.sizeof(capi.GatherSpeciesAdaptiveInfoPOD) == 64
    assert capi.GatherSpeciesAdaptiveInfoPOD.totalSamples.offset == 24 and capi.GatherSpeciesAdaptiveInfoPOD.walkedSamples.offset == 56
    info = capi.GatherSpeciesAdaptiveInfoPOD()
    assert info.as_dict(3) == {"rounds": 0, "unconverged": [0, 0, 0], "totalSamples": [0, 0, 0], "walkedSamples": 0}
    # the neighbours keep their arities and their info
    for name, arity in (("vr_gather_species_device", 9), ("vr_gather_species_sums_device", 12), ("vr_gather_angular_adaptive_device", 14),
                        ("vr_gather_adaptive_device", 13)):
        assert len(capi.SIGNATURES[name][1]) == arity, name
    assert ctypes.sizeof(capi.GatherAdaptiveInfoPOD) == 16
    sig = inspect.signature(vr.Trace.gatherSpeciesAdaptive)
    assert list(sig.parameters) == ["self", "target", "species", "reflection", "maxBounces", "minSamples", "maxSamples", "absTarget",
                                    "primFirst", "primCount", "returnInfo", "numpy"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert d["reflection"] is vr.GatherReflection.SPECULAR and d["maxBounces"] == 64 and d["minSamples"] == 64
    assert d["maxSamples"] == 4096 and d["absTarget"] == 0.0 and d["primFirst"] == 0 and d["primCount"] is None
    assert d["returnInfo"] is False and d["numpy"] is False
    assert vr.Trace._SPECIES_KEYS == {"sticking", "reflectivity", "cosinePower", "sourceLaw", "reflectivityLaw", "stickingLaw",
                                      "yieldLaw"}  # (the targets are arguments of the call, not species keys)
    hdr = open(os.path.join(ROOT, "include", "viennaray_amd", "viennaray.hpp")).read()
    for text in ("struct GatherSpeciesAdaptiveResult {",
                 "GatherSpeciesAdaptiveResult gatherSpeciesAdaptive(const std::vector<float> &relTargets",
                 "bool gatherSpeciesAdaptiveDevice("):
        assert text in hdr, text
    flags = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", os.path.join(ROOT, "include", "viennaray_amd"),
             "-I", os.path.join(ROOT, "include")]
    p = subprocess.run(["g++", "-fsyntax-only"] + flags + [os.path.join(ROOT, "tests", "aux", "facade_gather_species_adaptive.cpp")],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]


def test_kernel_file_shape():
    with open(os.path.join(INC, "vr_gather_species.hip")) as f:
        text = f.read()
    assert len(re.findall(r"__global__[^;{]*\bgather_species_decide_kernel\b", text)) == 1
    assert len(re.findall(r"__global__[^;{]*\bgather_species_kernel\b", text)) == 1
    assert re.search(r"template <int GEO, int D, int NS, int STAT>\s*__global__", text)
    assert sorted(set(re.findall(r"species_launch<(\d), (\d)>\(geo", text))) == [("2", "0"), ("2", "1"), ("4", "0"), ("4", "1")]
    assert len(re.findall(r"hipLaunchKernelGGL\(\(gather_species_kernel<", text)) == 4
    assert len(re.findall(r"pair_walk_lanes<", text)) == 1  # the walk appears once
    # the list and its masks are read in the STAT instantiations alone; the verdict is the header's function
    assert re.search(r"if constexpr \(STAT\) \{\s*if \(a\.list\) \{", text) and "sa.listMask[t]" in text
    assert "gather_species_decide(S1, S2," in text
    # the next list is placed by ballots and a prefix: no atomic on the list or the masks
    assert not re.search(r"atomic\w*\(\s*d\.next", text) and not re.search(r"atomic\w*\(\s*&?d\.nextMasks", text)
    with open(os.path.join(INC, "vr_gather.hip")) as f:
        assert "gather_species" not in f.read()
