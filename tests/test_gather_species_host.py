"""The species gather on the host (vr_gather_species*: several species weighed along one set of traced paths).  No GPU:
tests/aux/gather_species.cpp includes vr_gather.hpp alone — the per-species step the kernel compiles — and runs once plain
and once under AddressSanitizer and UndefinedBehaviorSanitizer, stand-alone.  Entry points, ctypes signatures, Python
signatures, the façade, the Makefile and the kernel file's shape are checked as the neighbours check theirs; vr_gather.hip
keeps every text its own tests pin."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "aux", "gather_species.cpp")
INC = os.path.join(ROOT, "viennaray_amd", "csrc")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-I", INC]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gather_species") / "gather_species")
    subprocess.check_call(["g++"] + FLAGS + [SRC, "-o", exe])
    return exe


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[-2000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "\n0 failed checks" in out.stdout
    m = re.search(r"^(\d+) checks$", out.stdout, flags=re.M)
    # 10^4 paths at NS = 2 and at NS = 4, several checks per species and vertex
    assert m and int(m.group(1)) >= 200_000, out.stdout[-2000:]
    return out


def test_every_species_is_its_single_path_bit_for_bit(program):
    _run(program)


def test_step_under_sanitizers(tmp_path):
    """the same program with ASan and UBSan, run stand-alone (nothing is loaded into python)"""
    exe = str(tmp_path / "gather_species_san")
    subprocess.check_call(["g++"] + FLAGS + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe])
    out = _run(exe)
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]


def test_host_program_takes_the_header_alone():
    text = open(SRC).read()
    assert re.findall(r'#include "([^"]+)"', text) == ["vr_gather.hpp"]
    assert re.search(r"\bint main\(", text)
    hpp = open(os.path.join(INC, "vr_gather.hpp")).read()
    for name in ("gather_species_absorb", "gather_species_reflect", "gather_species_step"):
        assert re.search(r"VR_GATHER_FN unsigned %s\(" % name, hpp), name  # host/device, returning the alive mask
    assert "GATHER_MAX_SPECIES = 4" in hpp


def test_entry_points_facade_and_python_methods_exist():
    import viennaray_amd as vr
    from viennaray_amd import capi

    txt = open(os.path.join(ROOT, "include", "viennaray_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"#define VR_GATHER_MAX_SPECIES 4u", code) and capi.VR_GATHER_MAX_SPECIES == 4
    L = vr.load()
    for name, arity in (("vr_gather_species_device", 9), ("vr_gather_species", 8), ("vr_gather_species_sums_device", 12),
                        ("vr_gather_species_sums", 11)):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
        assert decl and len(decl.group(1).split(",")) == arity, name
        assert "const vr_gather_spec *specs, const vr_gather_laws *laws, uint32_t numSpecies" in decl.group(1), name
        assert hasattr(L, name) and len(capi.SIGNATURES[name][1]) == arity, name
    # the two PODs a species is made of are the existing ones, unchanged
    assert ctypes.sizeof(capi.GatherSpecPOD) == 48 and ctypes.sizeof(capi.GatherLawsPOD) == 48
    # ... and so are the neighbours' arities
    for name, arity in (("vr_gather_angular_device", 8), ("vr_gather_angular", 7), ("vr_gather_angular_sums_device", 11),
                        ("vr_gather_angular_sums", 10), ("vr_debug_gather_angular_path", 13), ("vr_gather_paths_device", 11)):
        assert len(capi.SIGNATURES[name][1]) == arity, name
    sig = inspect.signature(vr.Trace.gatherSpecies)
    assert list(sig.parameters) == ["self", "samples", "species", "reflection", "maxBounces", "primFirst", "primCount", "numpy"]
    assert sig.parameters["reflection"].default is vr.GatherReflection.SPECULAR and sig.parameters["maxBounces"].default == 64
    assert sig.parameters["primFirst"].default == 0 and sig.parameters["primCount"].default is None
    assert sig.parameters["numpy"].default is False
    sig = inspect.signature(vr.Trace.gatherSpeciesSums)
    assert list(sig.parameters) == ["self", "chunkFirst", "chunks", "budget", "species", "reflection", "maxBounces", "primFirst",
                                    "primCount", "numpy"]
    assert vr.Trace._SPECIES_KEYS == {"sticking", "reflectivity", "cosinePower", "sourceLaw", "reflectivityLaw", "stickingLaw",
                                      "yieldLaw"}
    hdr = open(os.path.join(ROOT, "include", "viennaray_amd", "viennaray.hpp")).read()
    for text in ("struct GatherSpecies {", "gatherSpecies(unsigned samples, const std::vector<GatherSpecies> &species",
                 "bool gatherSpeciesDevice(", "bool gatherSpeciesSums("):
        assert text in hdr, text
    flags = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", os.path.join(ROOT, "include", "viennaray_amd"),
             "-I", os.path.join(ROOT, "include")]
    p = subprocess.run(["g++", "-fsyntax-only"] + flags + [os.path.join(ROOT, "tests", "aux", "facade_gather_species.cpp")],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]


def test_kernel_file_and_makefile():
    mk = open(os.path.join(INC, "Makefile")).read()
    api = re.search(r"^API_SRCS := (.*)$", mk, flags=re.M).group(1).split()
    hip = re.search(r"^HIP_SRCS := (.*)$", mk, flags=re.M).group(1).split()
    model = re.search(r"^MODEL_SRCS := (.*)$", mk, flags=re.M).group(1).split()
    assert "vr_gather_species.cpp" in api and "vr_gather_species.hip" in hip
    assert "vr_gather_species.hip" not in model and "vr_gather_device.hpp" not in model
    # the two share a stem: their objects must not
    assert "$(HIP_SRCS:%.hip=$(BUILD)/%.hip.o)" in mk and "$(BUILD)/%.hip.o: $(HERE)%.hip" in mk
    with open(os.path.join(INC, "vr_gather_species.hip")) as f:
        text = f.read()
    assert len(re.findall(r"__global__[^;{]*\bgather_species_kernel\b", text)) == 1
    assert len(re.findall(r"pair_walk_lanes<", text)) == 1  # the walk appears once
    assert re.search(r"template <int GEO, int D, int NS, int STAT>\s*__global__", text)
    for name in ("hit_walls(", "cast_segment(", "process_boundary_hit<D>(", "gather_species_absorb<NS>(", "gather_species_reflect<NS>(",
                 "gather_path_weight_laws(", "gather_q(", "gather_q2("):
        assert name in text, name
    # at most 16 instantiations: NS in {2, 4} x STAT, each over GEO x D in one helper
    assert sorted(set(re.findall(r"species_launch<(\d), (\d)>\(geo", text))) == [("2", "0"), ("2", "1"), ("4", "0"), ("4", "1")]
    assert len(re.findall(r"hipLaunchKernelGGL\(\(gather_species_kernel<", text)) == 4
    # the sums and the throughputs live in lane-private LDS slots, the laws are staged per species
    for decl in ("__shared__ float lawBuf[NS * 3 * GATHER_LAW_MAX]", "__shared__ float tS[NS * VR_BLOCK]",
                 "__shared__ long long sumS[NS * (1 + STAT) * VR_BLOCK]"):
        assert decl in text, decl
    assert "atomicAdd(&sumS" not in text and "atomicAdd(sumL" not in text


def test_gather_kernel_file_still_satisfies_its_pins():
    """vr_gather.hip lost five small helpers to vr_gather_device.hpp and nothing else"""
    with open(os.path.join(INC, "vr_gather.hip")) as f:
        text = f.read()
    assert len(re.findall(r"__global__[^;{]*\bgather_samples_kernel\b", text)) == 1
    assert len(re.findall(r"pair_walk_lanes<", text)) == 1
    assert re.search(r"template <int GEO, int D, bool REC, int PATH = 0, int STAT = 0>", text)
    for geo in (0, 1):
        for d in (2, 3):
            for tail in ("false>)", "true>)", "false, 1>)", "false, 2>)", "false, 0, 1>)", "false, 1, 1>)", "false, 3>)", "false, 3, 1>)"):
                assert "gather_samples_kernel<%d, %d, %s" % (geo, d, tail) in text, (geo, d, tail)
    assert not re.search(r"gather_samples_kernel<\d, \d, false, 4", text)  # no fourth family
    assert "gather_species" not in text
    assert re.search(r"__device__ __forceinline__ bool gather_bounce\(", text)
    assert '#include "vr_gather_device.hpp"' in text
    dev = open(os.path.join(INC, "vr_gather_device.hpp")).read()
    for name in ("V3 v3(", "void gather_primitive(", "V3 gather_hit_normal(", "u64 gather_draw(", "VR_GATHER_TNEAR = 1e-4f"):
        assert name in dev and name not in text, name
