"""The energy gather on the host (vr_gather_energy*: an ion's energy carried along a path, a yield by the arrival energy).
No GPU: tests/aux/gather_energy.cpp includes vr_gather.hpp alone — the arithmetic the kernel compiles — and runs once plain
and once under AddressSanitizer and UndefinedBehaviorSanitizer, stand-alone.  The energy draw and the source energy are
recomputed in numpy bit for bit.  Entry points, ctypes signatures, Python signatures, the façade, the Makefile and the kernel
file's shape are checked as the neighbours check theirs; vr_gather.hip and vr_gather_species.hip keep every text their own
tests pin."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "aux", "gather_energy.cpp")
INC = os.path.join(ROOT, "viennaray_amd", "csrc")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-pthread", "-I", INC]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gather_energy") / "gather_energy")
    subprocess.check_call(["g++"] + FLAGS + [SRC, "-o", exe])
    return exe


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[-2000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "\n0 failed checks" in out.stdout
    m = re.search(r"^(\d+) checks$", out.stdout, flags=re.M)
    # every M in 2 .. 256 with every Z0 in 2 .. M: 32 640 cases of 10^4 sequences, at least one check per step of each
    assert m and int(m.group(1)) >= 32_640 * 10_000 * 4, out.stdout[-2000:]
    return out


def test_cut_is_sound_and_retention_is_the_angular_throughput(program):
    _run(program)


def test_arithmetic_under_sanitizers(tmp_path):
    """the same program with ASan and UBSan, run stand-alone (nothing is loaded into python)"""
    exe = str(tmp_path / "gather_energy_san")
    subprocess.check_call(["g++"] + FLAGS + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe])
    out = _run(exe)
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]


# ---- the energy draw in numpy -------------------------------------------------------------------------------------------
def tea8(v0, v1):
    """vr_gather.hpp: gather_tea8 on uint32 arrays"""
    v0, v1 = np.asarray(v0, dtype=np.uint32).copy(), np.asarray(v1, dtype=np.uint32).copy()
    s0 = np.uint32(0)
    with np.errstate(over="ignore"):
        for _ in range(8):
            s0 = np.uint32((int(s0) + 0x9E3779B9) & 0xFFFFFFFF)
            v0 += ((v1 << np.uint32(4)) + np.uint32(0xA341316C)) ^ (v1 + s0) ^ ((v1 >> np.uint32(5)) + np.uint32(0xC8013EA4))
            v1 += ((v0 << np.uint32(4)) + np.uint32(0xAD90777D)) ^ (v0 + s0) ^ ((v0 >> np.uint32(5)) + np.uint32(0x7E95761E))
    return v0


def path_key(seed, prim, sample):
    with np.errstate(over="ignore"):
        return tea8(prim, (np.asarray(seed, dtype=np.uint32) ^ np.uint32(0x50415448)) + np.asarray(sample, dtype=np.uint32))


def energy_u(seed, prim, sample):
    key = path_key(seed, prim, sample)
    return (tea8(key, np.full(key.shape, 0x454E5247, dtype=np.uint32)) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def law(t, x):
    """vr_gather.hpp: gather_law in numpy float32, one operation per step"""
    t = np.asarray(t, dtype=np.float32)
    M = t.size
    x = np.asarray(x, dtype=np.float32)
    xc = np.minimum(np.maximum(np.where(np.isnan(x), np.float32(0), x), np.float32(0)), np.float32(1))
    xs = (xc * np.float32(M - 1)).astype(np.float32)
    k = np.minimum(xs.astype(np.int32), M - 2)
    f = (xs - k.astype(np.float32)).astype(np.float32)
    d = (t[k + 1] - t[k]).astype(np.float32)
    fd = (f * d).astype(np.float32)
    return (t[k] + fd).astype(np.float32)


def test_draw_and_source_energy_against_numpy(program):
    out = subprocess.run([program, "draws"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    rows = np.array([[int(v) for v in line.split()] for line in out.stdout.splitlines()], dtype=np.uint64)
    assert rows.shape == (10_000, 5)
    seed, prim, sample = (rows[:, c].astype(np.uint32) for c in range(3))
    u = energy_u(seed, prim, sample)
    assert np.array_equal(u.view(np.uint32), rows[:, 3].astype(np.uint32))
    assert u.min() >= 0.0 and u.max() < 1.0
    k = np.arange(37, dtype=np.float32)
    Q = (np.float32(10) + np.float32(2.5) * k + np.float32(0.125) * (k * k)).astype(np.float32)  # (exact in float32)
    assert np.array_equal(law(Q, u).view(np.uint32), rows[:, 4].astype(np.uint32))
    # the counter is "ENRG", beyond every bounce counter (2 x 65535 + 1)
    assert 0x454E5247 > 2 * 65535 + 1 and bytes.fromhex("454E5247") == b"ENRG"


def test_closed_form_reference_is_within_the_bound_of_a_numpy_estimator():
    """the GPU test's closed form (tests/test_gather_energy.py: direct flux / 4 per triangle, 5 sigma with sigma^2 =
    F (1 - F) / K) against the estimator itself run in numpy float64 on the trench's profile: K cosine-law directions per
    triangle, weight Y_E(u) where the direction reaches the opening.  The reference does not sit on the bound anywhere"""
    import closed_forms as cf
    g = cf.trench_mesh()
    cen, _ = cf.triangle_centroids(g)
    coord = np.where(g.part == cf.BOTTOM, cen[:, 0], cen[:, 2])
    n, K, w, d = len(g.tris), 4096, float(cf.W), float(cf.DEPTH)
    rng = np.random.default_rng(11)
    r1, r2, u = rng.random((3, n, K))
    a, b = np.sqrt(r2), np.sqrt(1.0 - r2) * np.cos(2.0 * np.pi * r1)  # along the normal, along the in-profile tangent
    part, c = g.part[:, None], coord[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        bottom = np.abs(c + b / a * d) < w / 2                      # from (x, -d) up to z = 0
        wall = (b > 0) & (a * (-c / b) < w)                         # from (-+w/2, z) across at most w before z = 0
    reach = np.where(part == cf.TOP, True, np.where(part == cf.BOTTOM, bottom, wall))
    weight = reach * np.maximum(0.0, 2.0 * u - 1.0)                 # energyYield [0, 0, 1] read at e = u
    got = weight.mean(axis=1)
    inside = g.part != cf.TOP
    F = np.ones(n)
    F[inside] = cf.radiosity(cf.W, cf.DEPTH, 1.0).direct_at(g.part[inside], coord[inside])[0]
    F = F / 4.0
    bound = 5.0 * np.sqrt(F * (1.0 - F) / K)
    use = np.abs(got - F) / bound
    print("numpy estimator: worst triangle uses %.0f %% of its bound" % (100 * use.max()))
    assert (bound > 0).all() and use.max() < 1.0


def test_host_program_takes_the_header_alone():
    text = open(SRC).read()
    assert re.findall(r'#include "([^"]+)"', text) == ["vr_gather.hpp"]
    assert re.search(r"\bint main\(", text)
    hpp = open(os.path.join(INC, "vr_gather.hpp")).read()
    for name in ("float gather_energy_u(", "float gather_energy_source(", "float gather_energy_retain(", "float gather_energy_arrival(",
                 "float gather_energy_weight(", "bool gather_energy_cut("):
        assert re.search(r"VR_GATHER_FN " + re.escape(name), hpp), name  # host/device
    assert "GATHER_ENERGY_COUNTER = 0x454E5247u" in hpp and "GATHER_END_ENERGY = 7" in hpp


ENTRY_POINTS = (("vr_gather_energy_device", 9), ("vr_gather_energy", 8), ("vr_gather_energy_sums_device", 12),
                ("vr_gather_energy_sums", 11), ("vr_gather_energy_adaptive_device", 15), ("vr_gather_energy_adaptive", 14),
                ("vr_debug_gather_energy_path", 15))


def test_entry_points_facade_and_python_methods_exist():
    import viennaray_amd as vr
    from viennaray_amd import capi

    txt = open(os.path.join(ROOT, "include", "viennaray_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"#define VR_GATHER_END_ENERGY 7", code) and vr.GatherEnd.ENERGY == 7
    L = vr.load()
    for name, arity in ENTRY_POINTS:
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
        assert decl and len(decl.group(1).split(",")) == arity, name
        head = re.sub(r"\s+", " ", decl.group(1))
        assert "const vr_gather_spec *spec, const vr_gather_laws *laws, const struct vr_gather_energy *energy, uint32_t prim" in head, name
        assert hasattr(L, name) and len(capi.SIGNATURES[name][1]) == arity, name
    # the POD: three (pointer, count, float) groups, the last float's place taken by energyCut
    assert ctypes.sizeof(capi.GatherEnergyPOD) == 48
    assert [f for f, _ in capi.GatherEnergyPOD._fields_] == ["energyYield", "energyYieldCount", "energyMax", "sourceQuantiles",
                                                            "sourceQuantilesCount", "sourceEnergy", "retentionLaw", "retentionCount",
                                                            "energyCut"]
    fields = re.search(r"struct vr_gather_energy \{(.*?)\};", code, flags=re.S).group(1)
    assert re.findall(r"(\w+);", fields) == [f for f, _ in capi.GatherEnergyPOD._fields_]
    # ... and the neighbours' PODs and arities are what they were
    assert ctypes.sizeof(capi.GatherSpecPOD) == 48 and ctypes.sizeof(capi.GatherLawsPOD) == 48
    for name, arity in (("vr_gather_angular_device", 8), ("vr_gather_angular", 7), ("vr_gather_angular_sums_device", 11),
                        ("vr_gather_angular_sums", 10), ("vr_gather_angular_adaptive", 13), ("vr_debug_gather_angular_path", 13),
                        ("vr_gather_paths_device", 11)):
        assert len(capi.SIGNATURES[name][1]) == arity, name
    angular = list(inspect.signature(vr.Trace.gatherAngular).parameters)[2:]
    sig = inspect.signature(vr.Trace.gatherEnergy)
    assert list(sig.parameters) == ["self", "samples", "energyYield", "energyMax", "sourceEnergy", "sourceQuantiles", "retentionLaw",
                                    "energyCut"] + angular
    assert sig.parameters["energyCut"].default is True and sig.parameters["sourceEnergy"].default is None
    assert sig.parameters["sourceQuantiles"].default is None and sig.parameters["retentionLaw"].default is None
    for name in ("gatherEnergyAdaptive", "gatherEnergySums", "debugGatherEnergyPath"):
        assert callable(getattr(vr.Trace, name)), name
    assert inspect.signature(vr.Trace.gatherEnergyAdaptive).parameters["energyCut"].default is True
    assert inspect.signature(vr.Trace.gatherEnergySums).parameters["energyCut"].default is True
    hdr = open(os.path.join(ROOT, "include", "viennaray_amd", "viennaray.hpp")).read()
    for text in ("struct GatherEnergy {", "gatherEnergy(unsigned samples, const GatherEnergy &energy", "bool gatherEnergyDevice(",
                 "bool gatherEnergySums(", "GatherAdaptiveResult gatherEnergyAdaptive(", "bool energyCut = true;"):
        assert text in hdr, text
    flags = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include", "-I", os.path.join(ROOT, "include", "viennaray_amd"),
             "-I", os.path.join(ROOT, "include")]
    p = subprocess.run(["g++", "-fsyntax-only"] + flags + [os.path.join(ROOT, "tests", "aux", "facade_gather_energy.cpp")],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]


def test_kernel_file_and_makefile():
    mk = open(os.path.join(INC, "Makefile")).read()
    api = re.search(r"^API_SRCS := (.*)$", mk, flags=re.M).group(1).split()
    hip = re.search(r"^HIP_SRCS := (.*)$", mk, flags=re.M).group(1).split()
    model = re.search(r"^MODEL_SRCS := (.*)$", mk, flags=re.M).group(1).split()
    assert "vr_gather_energy.cpp" in api and "vr_gather_energy.hip" in hip
    assert "vr_gather_energy.hip" not in model and "vr_gather_energy.cpp" not in model and "vr_gather_device.hpp" not in model
    with open(os.path.join(INC, "vr_gather_energy.hip")) as f:
        text = f.read()
    assert len(re.findall(r"__global__[^;{]*\bgather_energy_kernel\b", text)) == 1
    assert len(re.findall(r"pair_walk_lanes<", text)) == 1  # the walk appears once: the one-path walk is the same loop
    assert re.search(r"template <int GEO, int D, int STAT, bool ONE = false>\s*__global__", text)
    for name in ("hit_walls(", "cast_segment(", "process_boundary_hit<D>(", "gather_path_throughput(", "gather_path_throughput_law(",
                 "gather_path_weight_laws(", "gather_energy_u(", "gather_energy_source(", "gather_energy_retain(",
                 "gather_energy_arrival(", "gather_energy_cut(", "gather_energy_weight(", "gather_q(", "gather_q2("):
        assert name in text, name
    # the tables are staged in LDS beside the angular laws; E0 and P live in lane-private LDS slots
    for decl in ("__shared__ float lawBuf[3 * GATHER_LAW_MAX]", "__shared__ float energyBuf[3 * GATHER_LAW_MAX]",
                 "__shared__ float eS[2 * VR_BLOCK]"):
        assert decl in text, decl
    assert sorted(set(re.findall(r"gather_energy_kernel<(\d), (\d), (\w+)(?:, (\w+))?>\)", text))) == sorted(
        [(g, d, "STAT", "") for g in "01" for d in "23"] + [(g, d, "0", "true") for g in "01" for d in "23"])
    kernels = open(os.path.join(INC, "vr_kernels.hpp")).read()
    assert re.search(r"struct GatherEnergyArgs \{\s*GatherArgs a;", kernels)


def test_neighbour_kernel_files_still_satisfy_their_pins():
    """vr_gather.hip and vr_gather_species.hip know nothing of the energy: the new kernel is a translation unit of its own"""
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
    assert "gather_species" not in text and "energy" not in text.lower()
    assert re.search(r"__device__ __forceinline__ bool gather_bounce\(", text)
    with open(os.path.join(INC, "vr_gather_species.hip")) as f:
        species = f.read()
    assert "energy" not in species.lower()
    assert len(re.findall(r"hipLaunchKernelGGL\(\(gather_species_kernel<", species)) == 4
