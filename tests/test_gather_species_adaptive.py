"""gatherSpeciesAdaptive on the device (vr_gather_species_adaptive*; Trace.gatherSpeciesAdaptive): up to four species, each
to its own target error, along ONE set of traced paths.  The specification is an identity — row s of flux, stdErr and
samples has the bits of the single-species adaptive call of species s (gatherAngularAdaptive, gatherPathsAdaptive without
laws) under that species' own targets, for every s, S, order of the species, choice of the other species, range split,
entry point and launch shape — so every check here is bit for bit against the existing calls.  The targets are chosen so
that species stop at different K on the same primitive and some never converge: the masks are what is under test.  Then
walkedSamples, the relation to the fixed-K call, the refusals, and an apply left as it was.  The scenes and the species are
those of tests/test_gather_species.py, re-created here."""
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
MINS, MAXS = 64, 512  # three doublings
KINDS = [GR.SPECULAR, GR.DIFFUSE]
Y5 = np.linspace(0.5, 3.0, 5).astype(np.float32)
L5 = (np.linspace(0.0, 1.0, 5) ** 3).astype(np.float32)
# (relative, absolute) target of each species: distinct, one with an absolute target
TARGET = {"A": (0.05, 0.0), "B": (0.1, 0.0), "C": (0.08, 0.05), "D": (0.02, 0.0)}
LISTS = (("A", "B"), ("A", "B", "C"), ("A", "B", "C", "D"), ("D", "C", "B", "A"), ("C", "A", "C"))


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
    """A: rho 0.8.  B: 0 on the bottom, 0.9 elsewhere.  C: rho 1, R = [1, 0.2], Y = Y5.  D: rho 0.6 with the source law L5"""
    return {"A": dict(reflectivity=0.8), "B": dict(reflectivity=_table_b(scene)),
            "C": dict(reflectivity=1.0, reflectivityLaw=[1.0, 0.2], yieldLaw=Y5), "D": dict(reflectivity=0.6, sourceLaw=L5)}[name]


@functools.lru_cache(maxsize=None)
def _single(scene, kind, name, rel=None, abs_=None):
    """the adaptive call of one species alone over the whole scene — existing code, the reference: (flux, stdErr, samples,
    info), computed once, shared, read only"""
    t = _scene(scene)[0]
    rel, abs_ = (TARGET[name][0] if rel is None else rel), (TARGET[name][1] if abs_ is None else abs_)
    kw = dict(reflection=kind, maxBounces=MB, minSamples=MINS, maxSamples=MAXS, absTarget=abs_, returnInfo=True, numpy=True)
    call = t.gatherPathsAdaptive if name in ("A", "B") else t.gatherAngularAdaptive  # (no law: the path gather itself)
    flux, err, used, info = call(rel, **_species(scene, name), **kw)
    for a in (flux, err, used):
        a.setflags(write=False)
    return flux, err, used, info


def _call(scene, kind, names, **kw):
    t = _scene(scene)[0]
    kw.setdefault("numpy", True)
    return t.gatherSpeciesAdaptive([TARGET[n][0] for n in names], [_species(scene, n) for n in names], reflection=kind, maxBounces=MB,
                                   minSamples=MINS, maxSamples=MAXS, absTarget=[TARGET[n][1] for n in names], returnInfo=True, **kw)


def _same_rows(got, scene, kind, names, lo=0, hi=None):
    flux, err, used = got[:3]
    for s, name in enumerate(names):
        f, e, u, _ = _single(scene, kind, name)
        sl = slice(lo, hi)
        bad = np.nonzero((_bits(flux[s]) != _bits(f[sl])) | (_bits(err[s]) != _bits(e[sl])) | (used[s] != u[sl]))[0]
        assert len(bad) == 0, (scene, kind, names, name, [(int(i), float(flux[s][i]), float(f[sl][i]), int(used[s][i]), int(u[sl][i]))
                                                          for i in bad[:5]])


# ---------------------------------------------------------------------------------------------------------------
# 1. row identity
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["mesh", "disks2"])
@pytest.mark.parametrize("kind", KINDS)
def test_every_row_is_the_single_species_adaptive_call(scene, kind):
    n = len(_scene(scene)[1].part)
    # what the reference itself must show, or the masks are not exercised: at least three distinct K, primitives on which
    # two species stop at different K, primitives that are unconverged at maxSamples
    used = np.stack([_single(scene, kind, nm)[2] for nm in "ABCD"])
    infos = [_single(scene, kind, nm)[3] for nm in "ABCD"]
    ks = sorted(set(int(v) for v in np.unique(used)))
    print(scene, kind, "K:", {k: [int((used[s] == k).sum()) for s in range(4)] for k in ks}, "unconverged:",
          [i["unconverged"] for i in infos], "rounds:", [i["rounds"] for i in infos])
    assert len(ks) >= 3 and set(ks) <= {64, 128, 256, 512}, ks
    assert ((used[0] != used[1]) | (used[0] != used[2]) | (used[1] != used[2])).any()
    assert (used[0] != used[1]).any(), "A and B stop at the same K everywhere"
    assert sum(i["unconverged"] for i in infos) > 0 and (used < MAXS).any()
    for names in LISTS:
        got = _call(scene, kind, names)
        flux, err, samples, info = got
        for a, dt in ((flux, np.float32), (err, np.float32), (samples, np.uint32)):
            assert a.shape == (len(names), n) and a.dtype == dt
        _same_rows(got, scene, kind, names)
        ones = [_single(scene, kind, nm)[3] for nm in names]
        assert info["unconverged"] == [o["unconverged"] for o in ones], (names, info, ones)
        assert info["totalSamples"] == [o["totalSamples"] for o in ones], (names, info, ones)
        assert info["rounds"] == max(o["rounds"] for o in ones), (names, info, ones)
        assert info["totalSamples"] == [int(samples[s].sum()) for s in range(len(names))]
    # the species do differ: a kernel that copies row 0, or stops every species with the first, fails
    a, b = _single(scene, kind, "A"), _single(scene, kind, "B")
    assert (_bits(a[0]) != _bits(b[0])).any() and (a[0] > 0).any()


@pytest.mark.parametrize("scene", ["mesh", "disks2"])
def test_the_other_species_and_their_targets_do_not_matter(scene):
    """species A under its target beside a species that never converges (target 0), beside one that converges at once (a
    huge absolute target), and alone: the same bits"""
    t = _scene(scene)[0]
    kind = GR.SPECULAR
    f, e, u, info = _single(scene, kind, "A")
    sp = [_species(scene, "A"), _species(scene, "C")]
    kw = dict(reflection=kind, maxBounces=MB, minSamples=MINS, maxSamples=MAXS, returnInfo=True, numpy=True)
    for rel_c, abs_c in ((0.0, 0.0), (0.0, 1e6)):
        flux, err, used, inf = t.gatherSpeciesAdaptive([TARGET["A"][0], rel_c], sp, absTarget=[0.0, abs_c], **kw)
        assert (_bits(flux[0]) == _bits(f)).all() and (_bits(err[0]) == _bits(e)).all() and (used[0] == u).all()
        assert (used[1] == (MAXS if abs_c == 0.0 else MINS)).all()
        assert inf["unconverged"][1] == (len(f) if abs_c == 0.0 else 0) and inf["unconverged"][0] == info["unconverged"]
    # one species is the single call itself; a scalar target applies to every species
    flux, err, used, inf = t.gatherSpeciesAdaptive(TARGET["A"][0], [sp[0]], **kw)
    assert flux.shape == (1, len(f)) and (_bits(flux[0]) == _bits(f)).all() and (used[0] == u).all()
    assert inf == dict(rounds=info["rounds"], unconverged=[info["unconverged"]], totalSamples=[info["totalSamples"]],
                       walkedSamples=info["totalSamples"])
    flux, err, used, inf = t.gatherSpeciesAdaptive(0.1, [_species(scene, "B"), sp[0]], absTarget=0.01, **kw)
    for s, nm in enumerate(("B", "A")):
        w = _single(scene, kind, nm, 0.1, 0.01)
        assert (_bits(flux[s]) == _bits(w[0])).all() and (_bits(err[s]) == _bits(w[1])).all() and (used[s] == w[2]).all()
    with pytest.raises(ValueError):
        t.gatherSpeciesAdaptive([0.1, 0.1, 0.1], sp, **kw)  # three targets for two species


# ---------------------------------------------------------------------------------------------------------------
# 2. walkedSamples
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["mesh", "disks2"])
@pytest.mark.parametrize("kind", KINDS)
def test_walked_samples(scene, kind):
    for names in (("A", "B"), ("A", "B", "C", "D")):
        flux, err, samples, info = _call(scene, kind, names)
        assert info["walkedSamples"] == int(samples.max(axis=0).astype(np.int64).sum())
        assert info["walkedSamples"] <= sum(info["totalSamples"])
        assert info["walkedSamples"] < sum(info["totalSamples"])  # (S >= 2: every primitive shares round 0 at least)
        assert info["walkedSamples"] >= max(info["totalSamples"])
    flux, err, samples, info = _call(scene, kind, ("A", "A"))
    one = _single(scene, kind, "A")[3]
    assert info["walkedSamples"] == one["totalSamples"] and info["totalSamples"] == [one["totalSamples"]] * 2
    assert (_bits(flux[0]) == _bits(flux[1])).all() and (samples[0] == samples[1]).all()


# ---------------------------------------------------------------------------------------------------------------
# 3. range split and forms
# ---------------------------------------------------------------------------------------------------------------
def _raw(t, specs, laws, S, first, count, mins, maxs, rel, abs_, flux, err, used, info):
    f32, u32 = C.POINTER(C.c_float), C.POINTER(C.c_uint32)

    def ptr(a, ty):
        return a.ctypes.data_as(ty) if a is not None else None

    return t._L.vr_gather_species_adaptive(t._h, specs, laws, S, first, count, mins, maxs, ptr(rel, f32), ptr(abs_, f32), ptr(flux, f32),
                                           ptr(err, f32), ptr(used, u32), C.byref(info) if info is not None else None)


@pytest.mark.parametrize("scene", ["mesh", "disks2"])
@pytest.mark.parametrize("kind", KINDS)
def test_range_split_and_forms(scene, kind):
    import torch
    t, g = _scene(scene)
    n = len(g.part)
    names = ("A", "B", "C", "D")
    # 37: not a multiple of 64 — the second range starts inside a group of the whole range's
    cut = 37
    assert cut < n
    head = _call(scene, kind, names, primFirst=0, primCount=cut)
    tail = _call(scene, kind, names, primFirst=cut)
    _same_rows(head, scene, kind, names, 0, cut)
    _same_rows(tail, scene, kind, names, cut, n)
    whole = _call(scene, kind, names)
    for k in range(3):
        joined = np.concatenate([head[k], tail[k]], 1)
        assert joined.shape == (4, n) and (joined.view(np.uint32) == whole[k].view(np.uint32)).all()
    for key in ("unconverged", "totalSamples"):
        assert [a + b for a, b in zip(head[3][key], tail[3][key])] == whole[3][key]
    assert head[3]["walkedSamples"] + tail[3]["walkedSamples"] == whole[3]["walkedSamples"]
    one = _call(scene, kind, names, primFirst=n - 1)  # a range of one primitive
    _same_rows(one, scene, kind, names, n - 1, n)
    # the device form: a tensor table in, tensors out, on torch's current stream
    species = [_species(scene, nm) for nm in names]
    species[1] = dict(reflectivity=torch.from_numpy(_table_b(scene)).cuda())
    kw = dict(reflection=kind, maxBounces=MB, minSamples=MINS, maxSamples=MAXS, absTarget=[TARGET[nm][1] for nm in names], returnInfo=True)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dev = t.gatherSpeciesAdaptive([TARGET[nm][0] for nm in names], species, **kw)
        part = t.gatherSpeciesAdaptive([TARGET[nm][0] for nm in names], species, primFirst=cut, primCount=n - cut, **kw)
    stream.synchronize()
    for k, dt in enumerate((torch.float32, torch.float32, torch.int32)):
        assert isinstance(dev[k], torch.Tensor) and dev[k].is_cuda and dev[k].shape == (4, n) and dev[k].dtype == dt
        assert (dev[k].cpu().numpy().view(np.uint32) == whole[k].view(np.uint32)).all()
        assert (part[k].cpu().numpy().view(np.uint32) == whole[k][:, cut:].view(np.uint32)).all()
    assert dev[3] == whole[3] and part[3] == tail[3]
    # scalars alone: tensors unless numpy=True; three species run the four-wide kernel
    three = _call(scene, kind, ("A", "C", "D"), numpy=False)
    torch.cuda.synchronize()
    assert isinstance(three[0], torch.Tensor)
    _same_rows([a.cpu().numpy().view(dt) for a, dt in zip(three[:3], (np.float32, np.float32, np.uint32))], scene, kind, ("A", "C", "D"))
    with pytest.raises(ValueError):
        t.gatherSpeciesAdaptive(0.1, [species[1], _species(scene, "B")])  # tensors and numpy tables do not mix
    # stdErr = NULL and samplesUsed = NULL through the C entry point
    specs, laws, S, host, keep = t._speciesSpecs("test", [_species(scene, nm) for nm in names], kind, MB, True)
    rel = np.array([TARGET[nm][0] for nm in names], np.float32)
    abs_ = np.array([TARGET[nm][1] for nm in names], np.float32)
    for err, used in ((None, None), (np.empty((4, n), np.float32), None), (None, np.empty((4, n), np.uint32))):
        flux, info = np.full((4, n), -777.0, np.float32), capi.GatherSpeciesAdaptiveInfoPOD()
        assert _raw(t, specs, laws, 4, 0, n, MINS, MAXS, rel, abs_, flux, err, used, info) == capi.VR_OK
        assert (_bits(flux) == _bits(whole[0])).all() and info.as_dict(4) == whole[3]
        assert err is None or (_bits(err) == _bits(whole[1])).all()
        assert used is None or (used == whole[2]).all()


# ---------------------------------------------------------------------------------------------------------------
# 4. the relation to the fixed-K call
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["mesh", "disks2"])
@pytest.mark.parametrize("kind", KINDS)
def test_flux_is_the_fixed_k_species_call_at_the_k_it_stopped_at(scene, kind):
    t = _scene(scene)[0]
    names = ("A", "B", "C", "D")
    flux, err, samples, info = _call(scene, kind, names)
    seen = 0
    for k in sorted(set(int(v) for v in np.unique(samples))):
        rows = t.gatherSpecies(k, [_species(scene, nm) for nm in names], reflection=kind, maxBounces=MB, numpy=True)
        at = samples == k
        assert (_bits(flux)[at] == _bits(rows)[at]).all(), (scene, kind, k)
        seen += int(at.sum())
    assert seen == samples.size


# ---------------------------------------------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------------------------------------------
def _last(t):
    return t._L.vr_last_error(t._h).decode()


def test_refusals_leave_the_outputs_and_the_context_as_they_were():
    import torch
    t, g = _scene("mesh")
    n = len(g.part)
    poison = np.float32(-777.0)
    names = ("A", "B", "C", "D")
    species = [_species("mesh", nm) for nm in names]
    rel0 = np.array([TARGET[nm][0] for nm in names], np.float32)
    abs0 = np.array([TARGET[nm][1] for nm in names], np.float32)

    def pods(sp=species):
        specs, laws, S, host, keep = t._speciesSpecs("test", sp, GR.SPECULAR, MB, True)
        return specs, laws, keep

    def refused(specs, laws, S, text, first=0, count=n, mins=MINS, maxs=MAXS, rel=rel0, abs_=abs0, noinfo=False):
        flux, err = np.full((4, n), poison, np.float32), np.full((4, n), poison, np.float32)
        used = np.full((4, n), 12345, np.uint32)
        info = capi.GatherSpeciesAdaptiveInfoPOD(rounds=99)
        rc = _raw(t, specs, laws, S, first, count, mins, maxs, rel, abs_, flux, err, used, None if noinfo else info)
        assert rc == capi.VR_E_INVALID, text
        assert (flux == poison).all() and (err == poison).all() and (used == 12345).all() and info.rounds == 99, text
        assert text in _last(t), (text, _last(t))

    specs, laws, keep = pods()
    # the number of species, null arguments
    refused(specs, laws, 0, "numSpecies")
    refused(specs, laws, 5, "numSpecies")
    refused(None, laws, 4, "specs must not be null")
    refused(specs, laws, 4, "relTargets and absTargets must not be null", rel=None)
    refused(specs, laws, 4, "relTargets and absTargets must not be null", abs_=None)
    refused(specs, laws, 4, "info must not be null", noinfo=True)
    info = capi.GatherSpeciesAdaptiveInfoPOD()
    assert _raw(t, specs, laws, 4, 0, n, MINS, MAXS, rel0, abs0, None, None, None, info) == capi.VR_E_INVALID
    assert "out must not be null" in _last(t)
    # vr_gather_adaptive's rules for the sample counts
    refused(specs, laws, 4, "minSamples must be a positive multiple of 64", mins=0)
    refused(specs, laws, 4, "minSamples must be a positive multiple of 64", mins=100, maxs=400)
    refused(specs, laws, 4, "maxSamples must be minSamples times a power of two", maxs=192)
    refused(specs, laws, 4, "maxSamples must be minSamples times a power of two", mins=128, maxs=64)
    # a target of one species: the message names it
    for bad in (-0.1, float("nan")):
        rel = rel0.copy()
        rel[2] = bad
        refused(specs, laws, 4, "species 2: the targets must not be negative or NaN", rel=rel)
        abs_ = abs0.copy()
        abs_[3] = bad
        refused(specs, laws, 4, "species 3: the targets must not be negative or NaN", abs_=abs_)
    with pytest.raises(vr.VrError, match="species 1: the targets"):
        t.gatherSpeciesAdaptive([0.1, -1.0], species[:2], maxBounces=MB, minSamples=MINS, maxSamples=MAXS, numpy=True)
    # what vr_gather_species refuses, under the species' name, at samples = maxSamples
    for field, value in (("reflection", int(GR.DIFFUSE)), ("maxBounces", MB + 1)):
        specs, laws, keep = pods()
        setattr(specs[2], field, value)
        refused(specs, laws, 4, "species 2: reflection and maxBounces")
    specs, laws, keep = pods()
    specs[2].paths = 0
    refused(specs, laws, 4, "species 2: spec.paths must be 1")
    specs, laws, keep = pods()
    specs[1].reflectivity = None
    specs[1].reflectivityScalar = 1.5
    refused(specs, laws, 4, "species 1: the reflectivity must lie in [0, 1]")
    s2, l2, k2 = pods([species[0], dict(reflectivity=0.5, yieldLaw=[1.0, -2.0])])
    refused(s2, l2, 2, "species 1: yieldLaw[1]")
    specs, laws, keep = pods([species[0], species[1], species[2]])
    refused(specs, laws, 3, "species 2: samples x wbound", mins=1 << 21, maxs=1 << 21)  # Y up to 3 at 2^21 samples
    table = _table_b("mesh").copy()
    table[[17, 40]] = [np.float32(1.25), np.float32("nan")]
    sb, lb, kb = pods([species[0], dict(reflectivity=table), species[2]])
    refused(sb, lb, 3, "species 1: reflectivity[17]")
    with pytest.raises(vr.VrError, match=r"species 1: reflectivity\[17\]"):
        t.gatherSpeciesAdaptive(0.1, [species[0], dict(reflectivity=torch.from_numpy(table).cuda()), species[2]], maxBounces=MB,
                                minSamples=MINS, maxSamples=MAXS)
    # the range; nothing to do is VR_OK, after the checks
    specs, laws, keep = pods()
    flux = np.full((4, n), poison, np.float32)
    assert _raw(t, specs, laws, 4, 1, n, MINS, MAXS, rel0, abs0, flux, None, None, info) == capi.VR_E_INVALID and (flux == poison).all()
    assert _raw(t, specs, laws, 4, 0, 0, MINS, MAXS, rel0, abs0, None, None, None, info) == capi.VR_OK
    bad = rel0.copy()
    bad[0] = -1.0
    assert _raw(t, specs, laws, 4, 0, 0, MINS, MAXS, bad, abs0, None, None, None, info) == capi.VR_E_INVALID  # ... which come first
    # the device form refuses host memory and leaves device memory alone
    dev = torch.full((4, n), float(poison), device="cuda")
    host = np.full((4, n), poison, np.float32)
    f32 = C.POINTER(C.c_float)
    args = (specs, laws, 4, 0, n, MINS, MAXS, rel0.ctypes.data_as(f32), abs0.ctypes.data_as(f32))
    assert t._L.vr_gather_species_adaptive_device(t._h, *args, C.c_void_p(host.ctypes.data), None, None, C.byref(info),
                                                  None) == capi.VR_E_INVALID
    assert "device memory" in _last(t)
    specs[3].reflection = int(GR.DIFFUSE)
    assert t._L.vr_gather_species_adaptive_device(t._h, *args, C.c_void_p(dev.data_ptr()), None, None, C.byref(info),
                                                  None) == capi.VR_E_INVALID
    torch.cuda.synchronize()
    assert (host == poison).all() and bool((dev == float(poison)).all())
    # ... and the context still answers
    _same_rows(_call("mesh", GR.SPECULAR, names), "mesh", GR.SPECULAR, names)


def test_an_adaptive_species_gather_needs_what_a_prepare_left():
    g = cf.trench_mesh()
    t = _mesh_tracer(g)
    t.setParticleType(vr.DiffuseParticle(1.0, "flux"))
    t.setNumberOfRaysFixed(1000)
    t.setRngSeed(SEED)
    names = ("A", "B", "C")
    species = [_species("mesh", nm) for nm in names]
    kw = dict(maxBounces=MB, minSamples=MINS, maxSamples=MAXS, absTarget=[TARGET[nm][1] for nm in names], numpy=True)
    with pytest.raises(vr.VrError, match="nothing to gather from"):
        t.gatherSpeciesAdaptive([TARGET[nm][0] for nm in names], species, **kw)
    t.setMaxBoundaryHits(1 << 16)
    t.applyPrepare()
    got = t.gatherSpeciesAdaptive([TARGET[nm][0] for nm in names], species, **kw)  # (a fresh context: every work buffer grows here)
    _same_rows(got, "mesh", GR.SPECULAR, names)


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
        kw = dict(maxBounces=MB, minSamples=MINS, maxSamples=MAXS)
        t.gatherSpeciesAdaptive([0.05, 0.1, 0.2, 0.02], species, numpy=True, **kw)
        t.gatherSpeciesAdaptive(0.1, species[:2], reflection=GR.DIFFUSE, numpy=True, **kw)
        t.gatherSpeciesAdaptive(0.1, [species[0], species[2], species[3]], **kw)
        with pytest.raises(vr.VrError):
            t.gatherSpeciesAdaptive([0.1, -0.1], species[:2], **kw)
        assert (_bits(t.getLocalData().getVectorData("flux")) == _bits(first)).all()
    t.apply()
    return first, np.array(t.getLocalData().getVectorData("flux")), t.getRayTraceInfo().as_dict()


def test_an_apply_is_untouched_by_an_adaptive_species_gather():
    f0, s0, i0 = _apply_twice(False)
    f1, s1, i1 = _apply_twice(True)
    assert (_bits(f0) == _bits(f1)).all() and (_bits(s0) == _bits(s1)).all()
    skip = {"time", "timeBuild", "timeTrace", "timeTraceKernel", "timeGenKernel"}
    assert {k: v for k, v in i0.items() if k not in skip} == {k: v for k, v in i1.items() if k not in skip}


# ---------------------------------------------------------------------------------------------------------------
# 7. the C++ façade
# ---------------------------------------------------------------------------------------------------------------
def test_cpp_facade_gather_species_adaptive(tmp_path):
    """tests/aux/facade_gather_species_adaptive.cpp on a sheet of disks folded into V grooves; the flux rows it prints are
    the Python call's on the same scene, bit for bit"""
    flags = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include",
             "-I", os.path.join(ROOT, "include", "viennaray_amd"), "-I", os.path.join(ROOT, "include")]
    src = os.path.join(ROOT, "tests", "aux", "facade_gather_species_adaptive.cpp")
    exe = tmp_path / "facade_gather_species_adaptive"
    lib = os.path.join(ROOT, "viennaray_amd")
    subprocess.check_call(["g++", "-O1"] + flags + [src, "-o", str(exe), "-L", lib, "-lviennaray_amd",
                                                    "-L", "/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib,
                                                    "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "facade gather species adaptive ok" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
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
    flux, err, used = t.gatherSpeciesAdaptive(
        [0.05, 0.1, 0.2, 0.02], [dict(sticking=0.2), dict(reflectivity=table), dict(sticking=0.0, reflectivityLaw=[1.0, 0.2], yieldLaw=Y5),
                                 dict(sticking=0.4, cosinePower=8.0)],
        maxBounces=8, minSamples=MINS, maxSamples=MAXS, absTarget=[0.0, 0.0, 0.05, 0.0], numpy=True)
    assert len(printed) == 1 and printed[0].shape == (4 * n * n,)
    assert (_bits(printed[0]) == _bits(flux.ravel())).all()
