"""The catalogue of trace kernels (vr_types.hpp: mode_traits, trace_kernel_exists, trace_kernel_particle) on the host.  No
GPU: tests/aux/kernel_catalogue.cpp includes vr_types.hpp alone, prints the catalogue and checks (a) the counts of its sets —
67 kernels in the library's table, 18 in the statistics table, 10 / 8 in a lean / kNeedsFull module — and (c) the invariants
of every mode's traits; the same program runs once more built with AddressSanitizer and UndefinedBehaviorSanitizer,
stand-alone.  Here: (b) the catalogue's mangled names ARE the symbols of the device assembly of vr_trace.hip and
vr_trace_stats.hip whose name starts with trace_kernel, whatever follows — the table and the code object cannot drift apart,
and no kernel can stand beside the table under a name of its own — and (d) every (particle, mode) that
vr_prepare.cpp can ask for exists, for the geometry it asks it for, and the catalogue holds no kernel that nothing asks for."""
import itertools
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "viennaray_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "aux", "kernel_catalogue.cpp")
FLAGS = ["-O2", "-std=c++17", "-Wall", "-I", CSRC]
HIPCC = os.environ.get("VR_HIPCC", "/opt/rocm/bin/hipcc")
COUNTS = {"library": 67, "statistics": 18, "module_lean": 10, "module_full": 8, "module_lean_statistics": 10,
          "module_full_statistics": 8}
# enum TraceMode and the particle ids of vr_types.hpp
GENERAL, ABSORB_FLAT, ABSORB, GENERAL_FLAT, SMALL, ABSORB_RELIEF, GENERAL_RELIEF, RESUME, UNIFORM, PLANAR, PLANAR_ROUND, \
    LATTICE, LATTICE_LANES = range(13)
P_DIFFUSE, P_SPECULAR, P_EXT, P_EXT_FULL, P_EXT_STATS, P_EXT_FULL_STATS = range(6)


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "\n0 failed checks" in out.stdout and "FAILED" not in out.stdout
    return out


@pytest.fixture(scope="module")
def catalogue(tmp_path_factory):
    """the program's lines: {set: {(D, geo, particle, mode): mangled name}}, {mode: traits}, {(particle, mode): serving id}"""
    exe = str(tmp_path_factory.mktemp("catalogue") / "kernel_catalogue")
    subprocess.check_call(["g++"] + FLAGS + [SRC, "-o", exe])
    text = _run(exe).stdout
    print(text)
    sets, traits, served = {}, {}, {}
    for line in text.splitlines():
        w = line.split()
        if w[0] == "kernel":
            sets.setdefault(w[1], {})[tuple(int(v) for v in w[2:6])] = w[6]
        elif w[0] == "mode":
            traits[int(w[1])] = {k: int(v) for k, v in zip(w[2::2], w[3::2])}
        elif w[0] == "served":
            served[(int(w[1]), int(w[2]))] = int(w[3])
        elif w[0] == "count":
            assert len(sets.get(w[1], {})) == int(w[2])
    return sets, traits, served


def test_counts_and_traits(catalogue):
    sets, traits, served = catalogue
    assert {k: len(v) for k, v in sets.items()} == COUNTS  # (a)
    assert sorted(traits) == list(range(13)) and len(served) == 13 * 6
    for mode, t in traits.items():  # (c), once more from the printed lines
        assert t["base"] in (GENERAL, ABSORB_FLAT, ABSORB, GENERAL_FLAT), (mode, t)
        assert t["latticeLanes"] <= t["lattice"] <= t["planarRound"] <= t["planar"] <= t["uniform"] <= (t["base"] == ABSORB_FLAT), (mode, t)
        assert 1 <= t["waves"] <= 8, (mode, t)
        assert t["multiQueue"] == (t["base"] == GENERAL_FLAT) and t["xcdQueues"] == (mode == GENERAL_FLAT), (mode, t)
        assert t["spanBins"] == (16 if mode == GENERAL else 64 if mode in (GENERAL_FLAT, GENERAL_RELIEF) else 32), (mode, t)
        assert t["dynamicLds"] == (mode == SMALL), (mode, t)
    # the kernel's own defaults (vr_types.hpp: VR_*_WAVES) and the two fixed ones
    assert [traits[m]["waves"] for m in range(13)] == [6, 8, 7, 6, 5, 8, 6, 6, 8, 8, 8, 8, 8]


def test_catalogue_under_sanitizers(tmp_path):
    """the same program with ASan and UBSan, run stand-alone (nothing is loaded into python)"""
    exe = str(tmp_path / "kernel_catalogue_san")
    subprocess.check_call(["g++"] + FLAGS + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe])
    out = _run(exe)
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]


def test_catalogue_is_the_code_objects_symbols(catalogue, tmp_path):
    """(b) the device assembly of the two library units, compiled as the Makefile compiles them (both at once)"""
    assert os.path.isfile(HIPCC), "hipcc is needed: " + HIPCC
    sets = catalogue[0]
    units = {"library": "vr_trace.hip", "statistics": "vr_trace_stats.hip"}
    procs = {name: subprocess.Popen([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
                                     "-fno-fast-math", "-S", "--cuda-device-only", "-o", str(tmp_path / (name + ".s")),
                                     os.path.join(CSRC, unit)], stderr=subprocess.DEVNULL) for name, unit in units.items()}
    for name, proc in procs.items():
        assert proc.wait() == 0, units[name]
        asm = open(tmp_path / (name + ".s")).read()
        symbols = re.findall(r"^(_ZN2vr\d+trace_kernel\w*):", asm, flags=re.M)
        assert len(symbols) == len(set(symbols))
        assert set(symbols) == set(sets[name].values()), sorted(set(symbols) ^ set(sets[name].values()))
        assert len(symbols) == COUNTS[name]


# (d) What prepare asks for.  A row: the line of vr_prepare.cpp it mirrors (checked to be there still), the set, the
# geometries and the kernel particle ids (ParticleLaunch::kernelParticle) the line can meet, and the modes it asks for.
ANY_GEO = (0, 1)
DISKS = (0,)
BUILT_IN = (P_DIFFUSE, P_SPECULAR)  # an absorbing launch is never an extended one (choose_particle_kernel: `if (extended) L.absorb = false`)
REQUESTS = [
    # choose_trace_mode, the first choice: generalFlatOk is the catalogue's answer for MODE_GENERAL_FLAT ...
    ("L.traceMode = !L.absorb ? ((S.flatScene && generalFlatOk) ? MODE_GENERAL_FLAT : MODE_GENERAL) : (S.flatScene ? MODE_ABSORB_FLAT : MODE_ABSORB);",
     "library", (2, 3), DISKS, (P_DIFFUSE, P_SPECULAR, P_EXT, P_EXT_STATS), (GENERAL_FLAT,)),
    ("const bool generalFlatOk = !L.absorb && trace_kernel_exists(set, D, c->geo.geo, L.kernelParticle, MODE_GENERAL_FLAT);",
     "module", (2, 3), DISKS, (P_EXT, P_EXT_STATS), (GENERAL_FLAT,)),
    # ... MODE_GENERAL serves every particle on every geometry, the two absorbing modes the built-in particles
    ("L.traceMode = !L.absorb ?", "library", (2, 3), ANY_GEO, range(6), (GENERAL,)),
    ("L.traceMode = !L.absorb ?", "module", (2, 3), ANY_GEO, range(P_EXT, 6), (GENERAL,)),
    ("(S.flatScene ? MODE_ABSORB_FLAT : MODE_ABSORB);", "library", (2, 3), ANY_GEO, BUILT_IN, (ABSORB_FLAT, ABSORB)),
    ("L.traceMode = *K.absorbCarry ? MODE_ABSORB : MODE_ABSORB_FLAT;", "library", (2, 3), ANY_GEO, BUILT_IN, (ABSORB_FLAT, ABSORB)),
    ("L.traceMode = *K.generalFlat ? MODE_GENERAL_FLAT : MODE_GENERAL;", "library", (2, 3), DISKS,
     (P_DIFFUSE, P_SPECULAR, P_EXT, P_EXT_STATS), (GENERAL_FLAT, GENERAL)),
    # a scene with relief (build_relief_field: kernelOk is the catalogue's answer for the tight mode; never a run-time model):
    # the tight launch, and the loose one in the mode of the first choice, or MODE_RESUME
    ("L.traceMode = L.absorb ? MODE_ABSORB_RELIEF : MODE_GENERAL_RELIEF;", "library", (2, 3), ANY_GEO, BUILT_IN, (ABSORB_RELIEF, ABSORB)),
    ("L.traceMode = L.absorb ? MODE_ABSORB_RELIEF : MODE_GENERAL_RELIEF;", "library", (2, 3), DISKS, (P_DIFFUSE, P_SPECULAR, P_EXT),
     (GENERAL_RELIEF, GENERAL)),
    ("L.looseMode = MODE_RESUME;", "library", (2, 3), DISKS, (P_DIFFUSE, P_SPECULAR, P_EXT), (RESUME,)),
    # a scene that fits LDS: never absorbing (choose_particle_kernel: `if (S.smallScene) L.absorb = false`)
    ("L.traceMode = MODE_SMALL;", "library", (2, 3), ANY_GEO, range(6), (SMALL,)),
    ("L.traceMode = MODE_SMALL;", "module", (2, 3), ANY_GEO, range(P_EXT, 6), (SMALL,)),
    # the ladder of MODE_ABSORB_FLAT's variants (absorb_flat_kernel_mode, ParticleLaunch::kernelMode): 3-D disks, the library's.
    # The first row asks for nothing, it holds what `exists` is: the catalogue's answer; then a rung a row
    ("const auto exists = [&](int m) { return trace_kernel_exists(set, c->geo.D, c->geo.geo, trace_kernel_particle(L.kernelParticle, m), m); };",
     "library", (3,), DISKS, BUILT_IN, ()),
    ("!exists(MODE_ABSORB_FLAT_UNIFORM))", "library", (3,), DISKS, BUILT_IN, (UNIFORM,)),
    ("!exists(MODE_ABSORB_FLAT_PLANAR))", "library", (3,), DISKS, BUILT_IN, (PLANAR,)),
    ("!exists(MODE_ABSORB_FLAT_PLANAR_ROUND))", "library", (3,), DISKS, BUILT_IN, (PLANAR_ROUND,)),
    ("!exists(MODE_ABSORB_FLAT_LATTICE))", "library", (3,), DISKS, BUILT_IN, (LATTICE,)),
    ("!exists(MODE_ABSORB_FLAT_LATTICE_LANES))", "library", (3,), DISKS, BUILT_IN, (LATTICE_LANES,)),
]


def test_prepare_asks_for_nothing_else(catalogue):
    sets, traits, served = catalogue
    prepare = open(os.path.join(CSRC, "vr_prepare.cpp")).read()
    have = {"library": {**sets["library"], **sets["statistics"]},
            "module": {k: v for name, s in sets.items() if name.startswith("module_") for k, v in s.items()}}
    asked = {"library": set(), "module": set()}
    for line, which, dims, geos, particles, modes in REQUESTS:
        assert line in prepare, "vr_prepare.cpp no longer has the line this row mirrors: " + line
        for D, geo, particle, mode in itertools.product(dims, geos, particles, modes):
            key = (D, geo, served[(particle, mode)], mode)
            assert key in have[which], (line, which, D, geo, particle, mode)
            asked[which].add(key)
    # ... and the other way round: no kernel is compiled that no line above asks for
    for which in asked:
        assert asked[which] == set(have[which]), sorted(set(have[which]) - asked[which])
