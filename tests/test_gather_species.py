"""gatherSpecies on the device (vr_gather_species*; Trace.gatherSpecies, gatherSpeciesSums): up to four species weighed
along ONE set of traced paths.  The specification is an identity — row s has the bits of the single-species call of
species s (gatherAngular, gatherPaths without laws, gatherFlux at reflectivity 0) for every s, S, order of the species,
range split, entry point and launch shape — so every check here is bit for bit against the existing calls.  The species
are chosen to die at different vertices of the shared path; one (primitive, sample) where they provably do is looked up
with debugGatherAngularPath.  Then the sums, the refusals, and an apply left as it was.  The scenes are those of
tests/test_gather_angular.py, re-created here."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import viennaray_amd as vr
from viennaray_amd import capi
import closed_forms as cf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BC = vr.BoundaryCondition
GR = vr.GatherReflection
SEED = 7
MB = 8  # maxBounces: species C (rho = 1) would otherwise run to the default 64 on most paths
KINDS = [GR.SPECULAR, GR.DIFFUSE]
Y5 = np.linspace(0.5, 3.0, 5).astype(np.float32)
L5 = (np.linspace(0.0, 1.0, 5) ** 3).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _prepared(t):
    t.setParticleType(vr.DiffuseParticle(1.0, "flux"))
    t.setNumberOfRaysFixed(1000)
    t.setRngSeed(SEED)
    t.applyPrepare()
    return t


def _mesh_tracer(g):
    t = vr.TraceTriangle(3)
    t.setGeometry(g.verts, g.tris, 1.0)
    t.setBoundaryConditions([BC.REFLECTIVE_BOUNDARY, BC.PERIODIC_BOUNDARY, BC.REFLECTIVE_BOUNDARY])
    return t


@functools.lru_cache(maxsize=None)
def _scene(name):
    """(tracer, geometry): the trench mesh (320 triangles, 3-D) or the 2-D trench of disks"""
    if name == "mesh":
        g = cf.trench_mesh()
        t = _mesh_tracer(g)
        t.setMaxBoundaryHits(1 << 16)
        return _prepared(t), g
    g = cf.trench_disks(2)
    t = vr.TraceDisk(2)
    t.setGeometry(g.points, g.normals, 1.0)
    t.setBoundaryConditions([BC.REFLECTIVE_BOUNDARY, BC.REFLECTIVE_BOUNDARY])
    t.setSourceDirection(cf.POS_Y)
    return _prepared(t), g


@functools.lru_cache(maxsize=None)
def _table_b(scene):
    g = _scene(scene)[1]
    return np.where(np.asarray(g.part) == cf.BOTTOM, 0.0, 0.9).astype(np.float32)


def _species(scene, name):
    """A: rho 0.8.  B: 0 on the bottom, 0.9 elsewhere.  C: rho 1, R = [1, 0.2], Y = Y5.  D: rho 0.6 with the source law L5;
    E: rho 0.6 with cosinePower 8 and no law.  Z: rho 0 (the direct flux); ZY: rho 0 with Y5"""
    return {"A": dict(reflectivity=0.8), "B": dict(reflectivity=_table_b(scene)),
            "C": dict(reflectivity=1.0, reflectivityLaw=[1.0, 0.2], yieldLaw=Y5), "D": dict(reflectivity=0.6, sourceLaw=L5),
            "E": dict(reflectivity=0.6, cosinePower=8.0), "Z": dict(reflectivity=0.0),
            "ZY": dict(reflectivity=0.0, yieldLaw=Y5)}[name]


@functools.lru_cache(maxsize=None)
def _single(scene, samples, kind, name):
    """the single-species call of a species over the whole scene: computed once, shared, read only"""
    t = _scene(scene)[0]
    sp = _species(scene, name)
    if name in ("A", "B", "E", "Z"):  # no law: the path gather itself
        out = t.gatherPaths(samples, reflection=kind, maxBounces=MB, numpy=True, **sp)
    else:
        out = t.gatherAngular(samples, reflection=kind, maxBounces=MB, numpy=True, **sp)
    out.setflags(write=False)
    return out


def _rows(scene, samples, kind, names, **kw):
    t = _scene(scene)[0]
    return t.gatherSpecies(samples, [_species(scene, n) for n in names], reflection=kind, maxBounces=MB, numpy=True, **kw)


# ---------------------------------------------------------------------------------------------------------------
# 1. row identities
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["mesh", "disks2"])
@pytest.mark.parametrize("samples", [64, 100])
@pytest.mark.parametrize("kind", KINDS)
def test_every_row_is_the_single_species_call(scene, samples, kind):
    n = len(_scene(scene)[1].part)
    for names in (["A"], ["A", "B"], ["A", "B", "C"], ["A", "B", "C", "D"], ["E", "C", "B", "A"], ["B", "E"], ["D", "A", "E"]):
        rows = _rows(scene, samples, kind, names)
        assert rows.shape == (len(names), n) and rows.dtype == np.float32
        for s, name in enumerate(names):
            want = _single(scene, samples, kind, name)
            bad = np.nonzero(_bits(rows[s]) != _bits(want))[0]
            assert len(bad) == 0, (scene, samples, kind, names, name, [(int(i), float(rows[s][i]), float(want[i])) for i in bad[:5]])
    # the species do differ: a kernel that copies row 0 fails
    a, b = _single(scene, samples, kind, "A"), _single(scene, samples, kind, "B")
    assert (_bits(a) != _bits(b)).any() and (a > 0).any()
    # permuting the species permutes the rows; two identical species give identical rows
    fwd, rev = _rows(scene, samples, kind, ["A", "B", "C", "E"]), _rows(scene, samples, kind, ["E", "C", "B", "A"])
    assert (_bits(fwd) == _bits(rev[::-1])).all()
    twice = _rows(scene, samples, kind, ["C", "A", "C"])
    assert (_bits(twice[0]) == _bits(twice[2])).all() and (_bits(twice[0]) != _bits(twice[1])).any()


@pytest.mark.parametrize("scene", ["mesh", "disks2"])
@pytest.mark.parametrize("samples", [64, 100])
def test_a_species_of_reflectivity_zero_has_the_bits_of_gather_flux(scene, samples):
    t = _scene(scene)[0]
    flux = t.gatherFlux(samples, numpy=True)
    assert (flux > 0).any() and (flux < 1).any()
    for kind in KINDS:
        rows = _rows(scene, samples, kind, ["Z", "A", "ZY"])
        assert (_bits(rows[0]) == _bits(flux)).all()
        assert (_bits(rows[1]) == _bits(_single(scene, samples, kind, "A"))).all()  # ... while the path went on for A
        assert (rows[1] > flux).any()
        # times Y: the direct samples weighed by their own starting angle, the angular call at reflectivity 0
        assert (_bits(rows[2]) == _bits(_single(scene, samples, kind, "ZY"))).all()
        assert (_bits(rows[2]) != _bits(flux)).any()


# ---------------------------------------------------------------------------------------------------------------
# 2. species that die apart
# ---------------------------------------------------------------------------------------------------------------
def test_species_die_at_different_vertices_of_one_path():
    """one (primitive, sample < 64) of the mesh whose path under A has at least two more vertices than under B: B is
    absorbed on the bottom, A goes on from there — and the vertices they share are the same words.  The whole scene at
    K = 64 is what test_every_row_is_the_single_species_call compares, so this path is among them"""
    t, g = _scene("mesh")
    wall = np.nonzero(np.asarray(g.part) != cf.BOTTOM)[0]
    found = None
    for prim in wall[::7]:
        for sample in range(4):
            kw = dict(reflection=GR.SPECULAR, maxBounces=MB)
            pb = t.debugGatherAngularPath(int(prim), sample, reflectivity=_table_b("mesh"), **kw)
            if pb["end"] != capi.VR_GATHER_END_ABSORBED:
                continue
            pa = t.debugGatherAngularPath(int(prim), sample, reflectivity=0.8, **kw)
            if pa["numVertices"] >= pb["numVertices"] + 2:
                found = (int(prim), sample, pa, pb)
                break
        if found:
            break
    assert found, "no path of the sampled ones outlives species B by two vertices"
    prim, sample, pa, pb = found
    v = pb["numVertices"]
    assert (pa["ids"][:v] == pb["ids"]).all() and (_bits(pa["points"][:v]) == _bits(pb["points"])).all()
    assert pb["weight"] == 0 and pb["throughput"] == 0 and pa["throughput"] > 0
    # the rows of a call that holds this path are the single-species rows at that primitive (and everywhere else)
    rows = _rows("mesh", 64, GR.SPECULAR, ["A", "B"], primFirst=prim, primCount=1)
    assert _bits(rows[0])[0] == _bits(_single("mesh", 64, GR.SPECULAR, "A"))[prim]
    assert _bits(rows[1])[0] == _bits(_single("mesh", 64, GR.SPECULAR, "B"))[prim]


# ---------------------------------------------------------------------------------------------------------------
# 3. range split and forms
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["mesh", "disks2"])
@pytest.mark.parametrize("kind", KINDS)
def test_range_split_and_forms(scene, kind):
    import torch
    t, g = _scene(scene)
    n = len(g.part)
    names = ["A", "B", "C", "D"]
    want = np.stack([_single(scene, 100, kind, nm) for nm in names])
    # 65 = 1 + 64: a group of one lane, then a full group that does not start at a multiple of 64 (the 2-D trench has
    # fewer disks than that: there the second range is what is left of them)
    m = min(64, n - 1)
    assert scene != "mesh" or m == 64
    head = _rows(scene, 100, kind, names, primFirst=0, primCount=1)
    body = _rows(scene, 100, kind, names, primFirst=1, primCount=m)
    assert head.shape == (4, 1) and body.shape == (4, m)
    assert (_bits(np.concatenate([head, body], 1)) == _bits(want[:, :1 + m])).all()
    tail = _rows(scene, 100, kind, names, primFirst=n - 3)
    assert (_bits(tail) == _bits(want[:, n - 3:])).all()
    # the device form: a tensor table in, a tensor out, on torch's current stream
    species = [_species(scene, nm) for nm in names]
    species[1] = dict(reflectivity=torch.from_numpy(_table_b(scene)).cuda())
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dev = t.gatherSpecies(100, species, reflection=kind, maxBounces=MB)
        part = t.gatherSpecies(100, species, reflection=kind, maxBounces=MB, primFirst=1, primCount=m)
    stream.synchronize()
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and dev.shape == (4, n) and dev.dtype == torch.float32
    assert (_bits(dev.cpu().numpy()) == _bits(want)).all()
    assert (_bits(part.cpu().numpy()) == _bits(want[:, 1:1 + m])).all()
    # scalars alone: a tensor unless numpy=True; three species run the four-wide kernel
    three = t.gatherSpecies(100, [_species(scene, nm) for nm in ("A", "C", "E")], reflection=kind, maxBounces=MB)
    torch.cuda.synchronize()
    assert isinstance(three, torch.Tensor)
    assert (_bits(three.cpu().numpy()) == _bits(np.stack([_single(scene, 100, kind, nm) for nm in ("A", "C", "E")]))).all()
    # tensors and numpy tables do not mix; unknown keys are refused
    with pytest.raises(ValueError):
        t.gatherSpecies(64, [species[1], _species(scene, "B")])
    with pytest.raises(ValueError):
        t.gatherSpecies(64, [dict(reflectivity=0.8, coneLaw=[1.0, 1.0])])
    with pytest.raises(ValueError):
        t.gatherSpecies(64, [dict(yieldLaw=Y5)])  # neither sticking nor reflectivity


# ---------------------------------------------------------------------------------------------------------------
# 4. the sums
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["mesh", "disks2"])
@pytest.mark.parametrize("kind", KINDS)
def test_sums_are_the_angular_sums_and_add(scene, kind):
    import torch
    t, g = _scene(scene)
    n = len(g.part)
    names = ["A", "B", "C", "D"]
    species = [_species(scene, nm) for nm in names]
    kw = dict(reflection=kind, maxBounces=MB, numpy=True)
    s1, s2 = t.gatherSpeciesSums(0, 2, 128, species, **kw)
    assert s1.shape == (4, n) and s2.shape == (4, n) and s1.dtype == np.int64 and s2.dtype == np.int64
    for s, sp in enumerate(species):
        a1, a2 = t.gatherAngularSums(0, 2, 128, **sp, **kw)
        assert (s1[s] == a1).all() and (s2[s] == a2).all(), (scene, kind, names[s])
    assert (s1[0] != s1[1]).any() and (s2[2] > 0).any()
    # adjacent chunk ranges add; a range of the primitives is that range of the rows
    lo = t.gatherSpeciesSums(0, 1, 128, species, **kw)
    hi = t.gatherSpeciesSums(1, 1, 128, species, **kw)
    assert (lo[0] + hi[0] == s1).all() and (lo[1] + hi[1] == s2).all()
    m = min(64, n - 1)
    p1, p2 = t.gatherSpeciesSums(0, 2, 128, species, primFirst=1, primCount=m, **kw)
    assert (p1 == s1[:, 1:1 + m]).all() and (p2 == s2[:, 1:1 + m]).all()
    # (float)(sum / 2^40 / K) over chunks [0, K / 64) with budget K is the fixed-K row
    rows = _rows(scene, 128, kind, names)
    assert (_bits((s1.astype(np.float64) / 2.0 ** 40 / 128).astype(np.float32)) == _bits(rows)).all()
    # one species goes to the angular sums; the device form gives tensors
    o1, o2 = t.gatherSpeciesSums(0, 2, 128, [species[2]], **kw)
    assert (o1[0] == s1[2]).all() and (o2[0] == s2[2]).all()
    d1, d2 = t.gatherSpeciesSums(0, 2, 128, [species[0], species[2], species[3]], reflection=kind, maxBounces=MB)
    torch.cuda.synchronize()
    assert isinstance(d1, torch.Tensor) and d1.dtype == torch.int64 and d1.shape == (3, n)
    assert (d1.cpu().numpy() == s1[[0, 2, 3]]).all() and (d2.cpu().numpy() == s2[[0, 2, 3]]).all()
    z1, z2 = t.gatherSpeciesSums(0, 0, 128, species, **kw)  # no chunk: zeros
    assert not z1.any() and not z2.any()


# ---------------------------------------------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------------------------------------------
def _raw(t, specs, laws, S, first, count, samples, out):
    ptr = out.ctypes.data_as(C.POINTER(C.c_float)) if out is not None else None
    return t._L.vr_gather_species(t._h, specs, laws, S, first, count, samples, ptr)


def _last(t):
    return t._L.vr_last_error(t._h).decode()


def test_refusals_leave_the_outputs_and_the_context_as_they_were():
    import torch
    t, g = _scene("mesh")
    n = len(g.part)
    poison = np.float32(-777.0)
    names = ["A", "B", "C", "D"]
    species = [_species("mesh", nm) for nm in names]
    want = np.stack([_single("mesh", 64, GR.SPECULAR, nm) for nm in names])

    def pods(sp=species):
        specs, laws, S, host, keep = t._speciesSpecs("test", sp, GR.SPECULAR, MB, True)
        return specs, laws, keep

    def refused(specs, laws, S, first=0, count=n, samples=64, text=None):
        out = np.full((max(S, 1), n), poison, np.float32)
        assert _raw(t, specs, laws, S, first, count, samples, out) == capi.VR_E_INVALID, text
        assert (out == poison).all(), text
        if text:
            assert text in _last(t), (text, _last(t))

    specs, laws, keep = pods()
    out = np.full((4, n), poison, np.float32)
    assert _raw(t, specs, laws, 4, 0, n, 64, out) == capi.VR_OK and (_bits(out) == _bits(want)).all()  # (the raw call works)
    # the number of species
    refused(specs, laws, 0, text="numSpecies")
    five = [_species("mesh", "A")] * 5
    s5, l5, k5 = pods(five)
    refused(s5, l5, 5, text="numSpecies")
    with pytest.raises(vr.VrError, match="numSpecies"):
        t.gatherSpecies(64, [])
    with pytest.raises(vr.VrError, match="numSpecies"):
        t.gatherSpecies(64, five)
    # what the species share: the first species that differs from species 0 is named
    for field, value in (("reflection", int(GR.DIFFUSE)), ("maxBounces", MB + 1)):
        specs, laws, keep = pods()
        setattr(specs[2], field, value)
        setattr(specs[3], field, value)
        refused(specs, laws, 4, text="species 2: reflection and maxBounces")
    emission = np.zeros(n, np.float32)
    for field, value in (("paths", 0), ("paths", 2), ("mode", capi.VR_GATHER_SOURCE), ("emission", emission.ctypes.data)):
        specs, laws, keep = pods()
        setattr(specs[2], field, value)
        refused(specs, laws, 4, text="species 2: spec.paths must be 1")
    # per species: what the angular call refuses, under the species' name
    specs, laws, keep = pods()
    specs[1].reflectivity = None
    specs[1].reflectivityScalar = 1.5
    refused(specs, laws, 4, text="species 1: the reflectivity must lie in [0, 1]")
    specs, laws, keep = pods()
    specs[3].cosinePower = 2.0
    refused(specs, laws, 4, text="species 3: a sourceLaw takes the place of the power cosine")
    s2, l2, k2 = pods([species[0], dict(reflectivity=0.5, yieldLaw=[1.0, -2.0])])
    refused(s2, l2, 2, text="species 1: yieldLaw[1]")
    # samples x wbound_s <= 2^22, per species: Y up to 3 is too much at 2^21 samples for species 2 alone
    specs, laws, keep = pods([species[0], species[1], species[2]])
    refused(specs, laws, 3, samples=1 << 21, text="species 2: samples x wbound")
    with pytest.raises(vr.VrError, match="species 1: samples x g"):
        t.gatherSpecies(1 << 20, [dict(reflectivity=0.8), dict(reflectivity=0.8, cosinePower=16.0)])
    # a bad reflectivity table in species 1: species and lowest index
    table = _table_b("mesh").copy()
    table[[17, 40]] = [np.float32(1.25), np.float32("nan")]
    sb, lb, kb = pods([species[0], dict(reflectivity=table), species[2]])
    refused(sb, lb, 3, text="species 1: reflectivity[17]")
    dev_out = torch.full((3, n), float(poison), device="cuda")
    with pytest.raises(vr.VrError, match=r"species 1: reflectivity\[17\]"):
        t.gatherSpecies(64, [species[0], dict(reflectivity=torch.from_numpy(table).cuda()), species[2]], maxBounces=MB)
    # null specs / out, the range
    specs, laws, keep = pods()
    refused(None, laws, 4, text="specs must not be null")
    assert _raw(t, specs, laws, 4, 0, n, 64, None) == capi.VR_E_INVALID and "out must not be null" in _last(t)
    refused(specs, laws, 4, first=1, count=n)
    assert _raw(t, specs, laws, 4, 0, 0, 64, None) == capi.VR_OK  # nothing to do, after the checks
    sz, lz, kz = pods([species[0], dict(reflectivity=0.5, yieldLaw=[1.0, -2.0])])
    assert _raw(t, sz, lz, 2, 0, 0, 64, None) == capi.VR_E_INVALID  # ... which come first
    assert _raw(t, specs, None, 4, 0, n, 64, out) == capi.VR_OK  # laws NULL: no species has a law
    for s, nm in enumerate(("A", "B")):
        assert (_bits(out[s]) == _bits(want[s])).all()
    # the device form refuses host memory and leaves device memory alone; the sums refuse the same and a range beyond the budget
    sd, ld, kd = pods([species[0], species[2]])
    host = np.full((2, n), poison, np.float32)
    assert t._L.vr_gather_species_device(t._h, sd, ld, 2, 0, n, 64, C.c_void_p(host.ctypes.data), None) == capi.VR_E_INVALID
    sd[1].reflection = int(GR.DIFFUSE)
    assert t._L.vr_gather_species_device(t._h, sd, ld, 2, 0, n, 64, C.c_void_p(dev_out.data_ptr()), None) == capi.VR_E_INVALID
    torch.cuda.synchronize()
    assert (host == poison).all() and bool((dev_out == float(poison)).all())
    with pytest.raises(vr.VrError, match="beyond the budget"):
        t.gatherSpeciesSums(1, 2, 128, species, maxBounces=MB, numpy=True)
    with pytest.raises(vr.VrError, match="species 1: yieldLaw"):
        t.gatherSpeciesSums(0, 1, 64, [species[0], dict(reflectivity=0.5, yieldLaw=[1.0, -2.0])], numpy=True)
    i64 = C.POINTER(C.c_int64)
    sums = np.full((4, n), -5, np.int64)
    assert t._L.vr_gather_species_sums(t._h, specs, laws, 4, 0, n, 0, 1, 64, sums.ctypes.data_as(i64), None) == capi.VR_E_INVALID
    assert (sums == -5).all()
    # ... and the context still answers
    assert (_bits(_rows("mesh", 64, GR.SPECULAR, names)) == _bits(want)).all()


def test_a_species_gather_needs_what_a_prepare_left():
    g = cf.trench_mesh()
    t = _mesh_tracer(g)
    t.setParticleType(vr.DiffuseParticle(1.0, "flux"))
    t.setNumberOfRaysFixed(1000)
    t.setRngSeed(SEED)
    species = [_species("mesh", nm) for nm in ("A", "B", "C")]
    with pytest.raises(vr.VrError, match="nothing to gather from"):
        t.gatherSpecies(64, species, maxBounces=MB, numpy=True)
    t.setMaxBoundaryHits(1 << 16)
    t.applyPrepare()
    got = t.gatherSpecies(64, species, maxBounces=MB, numpy=True)  # (a fresh context: every work buffer grows here)
    for s, nm in enumerate(("A", "B", "C")):
        assert (_bits(got[s]) == _bits(_single("mesh", 64, GR.SPECULAR, nm))).all()


# ---------------------------------------------------------------------------------------------------------------
# 6. an apply is untouched
# ---------------------------------------------------------------------------------------------------------------
def _apply_twice(gather_between):
    g = cf.trench_mesh()
    t = _mesh_tracer(g)
    t.setParticleType(vr.DiffuseParticle(0.3, "flux"))
    t.setNumberOfRaysFixed(200_000)
    t.setRngSeed(SEED)
    t.setUseRandomSeeds(False)
    t.apply()
    first = np.array(t.getLocalData().getVectorData("flux"))
    if gather_between:
        species = [_species("mesh", nm) for nm in ("A", "B", "C", "D")]
        t.gatherSpecies(128, species, maxBounces=MB, numpy=True)
        t.gatherSpecies(64, species[:2], reflection=GR.DIFFUSE, maxBounces=MB, numpy=True)
        t.gatherSpecies(64, [species[0], species[2], species[3]])
        t.gatherSpeciesSums(0, 1, 64, species, maxBounces=MB, numpy=True)
        with pytest.raises(vr.VrError):
            t.gatherSpecies(64, [species[0], dict(reflectivity=0.8, yieldLaw=[-1.0, 1.0])])
        assert (_bits(t.getLocalData().getVectorData("flux")) == _bits(first)).all()
    t.apply()
    return first, np.array(t.getLocalData().getVectorData("flux")), t.getRayTraceInfo().as_dict()


def test_an_apply_is_untouched_by_a_species_gather():
    f0, s0, i0 = _apply_twice(False)
    f1, s1, i1 = _apply_twice(True)
    assert (_bits(f0) == _bits(f1)).all() and (_bits(s0) == _bits(s1)).all()
    skip = {"time", "timeBuild", "timeTrace", "timeTraceKernel", "timeGenKernel"}
    assert {k: v for k, v in i0.items() if k not in skip} == {k: v for k, v in i1.items() if k not in skip}


# ---------------------------------------------------------------------------------------------------------------
# 7. the C++ façade
# ---------------------------------------------------------------------------------------------------------------
def test_cpp_facade_gather_species(tmp_path):
    """tests/aux/facade_gather_species.cpp on a sheet of disks folded into V grooves; the rows it prints are the Python
    call's on the same scene, bit for bit"""
    flags = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include",
             "-I", os.path.join(ROOT, "include", "viennaray_amd"), "-I", os.path.join(ROOT, "include")]
    src = os.path.join(ROOT, "tests", "aux", "facade_gather_species.cpp")
    exe = tmp_path / "facade_gather_species"
    lib = os.path.join(ROOT, "viennaray_amd")
    subprocess.check_call(["g++", "-O1"] + flags + [src, "-o", str(exe), "-L", lib, "-lviennaray_amd",
                                                    "-L", "/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib,
                                                    "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "facade gather species ok" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    printed = [np.array([float.fromhex(v) for v in line.split()[1:]], np.float32)
               for line in out.stdout.splitlines() if line.startswith("rows")]
    import math
    n = 16
    pts, nrm = [], []
    for i in range(n):
        for j in range(n):
            k = i % 8
            s = -1.0 if k < 4 else 1.0
            pts.append([float(i), float(j), 1.5 * abs(k - 4)])
            nrm.append([-s * 1.5 / math.sqrt(3.25), 0.0, 1.0 / math.sqrt(3.25)])
    t = vr.TraceDisk(3)
    t.setGeometry(np.array(pts, np.float32), np.array(nrm, np.float32), 1.0)
    t.setBoundaryConditions([BC.PERIODIC_BOUNDARY] * 3)
    _prepared(t)
    table = np.full(n * n, 0.9, np.float32)
    table[::3] = 0.0
    got = t.gatherSpecies(100, [dict(sticking=0.2), dict(reflectivity=table),
                                dict(sticking=0.0, reflectivityLaw=[1.0, 0.2], yieldLaw=Y5), dict(sticking=0.4, cosinePower=8.0)],
                          maxBounces=8, numpy=True)
    assert len(printed) == 1 and printed[0].shape == (4 * n * n,)
    assert (_bits(printed[0]) == _bits(got.ravel())).all()
