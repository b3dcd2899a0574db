"""The gather to a target error on the device (vr_gather_sums*, vr_gather_adaptive*; include/viennaray_amd.h has the
definition): the exact int64 sums of the weights and of their squares over a range of chunks, and the adaptive call built
on them.  Everything here is an identity or a replay: the sums divide to the fixed-K calls bit for bit, add over chunk
splits and do not depend on range splits or on how a chunk is cut into work items; the squares are those of the weights
vr_debug_gather_path reports; the adaptive call's every decision is the numpy rule of tests/test_gather_adaptive_host.py
(which that file shows to be the header's, bit for bit) applied to sums the sums call returns, and its flux is the fixed-K
flux at the sample count it reports.  One statistical test: over 16 seeds the reported squared error is the variance of the
estimate.  The scenes are those of tests/closed_forms.py and trenchGrid2D.dat; no sample count exceeds 1024."""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import viennaray_amd as vr
from viennaray_amd import capi
import closed_forms as cf
from helpers import trench2d
from test_gather_adaptive_host import np_converged, np_moments

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BC = vr.BoundaryCondition
GM = vr.GatherMode
GR = vr.GatherReflection
SEED = 7
POISON = np.float32(-123.5)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _prepared(t, seed=SEED):
    t.setParticleType(vr.DiffuseParticle(1.0, "flux"))
    t.setNumberOfRaysFixed(1000)
    t.setRngSeed(seed)
    t.applyPrepare()
    return t


def _mesh_tracer(g):
    t = vr.TraceTriangle(3)
    t.setGeometry(g.verts, g.tris, 1.0)
    t.setBoundaryConditions([BC.REFLECTIVE_BOUNDARY, BC.PERIODIC_BOUNDARY, BC.REFLECTIVE_BOUNDARY])
    return t


@functools.lru_cache(maxsize=None)
def _scene(name):
    """(tracer, number of primitives, part of every primitive or None)"""
    if name == "mesh":
        g = cf.trench_mesh()
        return _prepared(_mesh_tracer(g)), len(g.tris), g.part
    if name == "disks2":
        g = cf.trench_disks(2)
        t = vr.TraceDisk(2)
        t.setGeometry(g.points, g.normals, 1.0)
        t.setBoundaryConditions([BC.REFLECTIVE_BOUNDARY, BC.REFLECTIVE_BOUNDARY])
        t.setSourceDirection(cf.POS_Y)
        return _prepared(t), len(g.points), g.part
    if name == "disks3":  # 81 rows of the trench profile: more primitives than one block of the decide kernel takes
        g = cf.trench_disks(3, ny=80)
        t = vr.TraceDisk(3)
        t.setGeometry(g.points, g.normals, 1.0)
        t.setBoundaryConditions([BC.REFLECTIVE_BOUNDARY, BC.PERIODIC_BOUNDARY, BC.REFLECTIVE_BOUNDARY])
        return _prepared(t), len(g.points), g.part
    gd, p, n = trench2d()
    t = vr.TraceDisk(2)
    t.setGeometry(p, n, gd)
    t.setSourceDirection(vr.TraceDirection.POS_Y)
    t.setBoundaryConditions([BC.PERIODIC_BOUNDARY] * 2)
    return _prepared(t), len(p), None


SCENES = ["mesh", "disks2", "grid2"]


def _emission(n):
    return (0.25 + 0.5 * np.random.default_rng(5).random(n)).astype(np.float32)


# what a sample is: name -> (fixed-K call, sums call, adaptive call), each taking the tracer and the call's own arguments
def _kind(name, n):
    if name in ("specular", "diffuse"):
        kw = dict(reflectivity=0.7, reflection=GR.SPECULAR if name == "specular" else GR.DIFFUSE, maxBounces=16)
        return (lambda t, K, **r: t.gatherPaths(K, numpy=True, **kw, **r),
                lambda t, c0, c, b, **r: t.gatherPathsSums(c0, c, b, numpy=True, **kw, **r),
                lambda t, target, **r: t.gatherPathsAdaptive(target, numpy=True, **kw, **r), 1.0)
    kw = {"normal1": dict(cosinePower=1.0), "normal8": dict(cosinePower=8.0), "source8": dict(cosinePower=8.0, mode=GM.SOURCE),
          "emission": dict(cosinePower=1.0, emission=_emission(n))}[name]
    return (lambda t, K, **r: t.gatherFlux(K, numpy=True, **kw, **r),
            lambda t, c0, c, b, **r: t.gatherFluxSums(c0, c, b, numpy=True, **kw, **r),
            lambda t, target, **r: t.gatherFluxAdaptive(target, numpy=True, **kw, **r), float(kw["cosinePower"]))


KINDS = ["normal1", "normal8", "source8", "emission", "specular", "diffuse"]


def _result(s1, K):
    """gather_result: (float)((double)sum / 2^40 / K)"""
    return (s1.astype(np.float64) / 2.0 ** 40 / np.asarray(K, dtype=np.float64)).astype(np.float32)


def _g(power, D):
    """g_D(n) as the library takes it: a float32"""
    if power == 1.0:
        return 1.0
    if D == 3:
        return (power + 1) / 2
    return float(np.float32(2.0 / (math.sqrt(math.pi) * math.exp(math.lgamma((power + 1) / 2) - math.lgamma(power / 2 + 1)))))


def _np_q2(w, wmax):
    w = np.asarray(w, dtype=np.float32)
    wc = np.minimum(np.minimum(w, np.float32(wmax)), np.float32(2048)).astype(np.float64)
    return np.where(w > 0, np.floor(wc * wc * 2.0 ** 28 + 0.5), 0.0).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------
# 1. the sums against the fixed-K calls
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", SCENES)
@pytest.mark.parametrize("kind", KINDS)
def test_sums_divide_to_the_fixed_k_call(scene, kind):
    t, n, _ = _scene(scene)
    fixed, sums, _, _ = _kind(kind, n)
    for K in (64, 192):  # (192: three chunks, wmax that of 256)
        s1, s2 = sums(t, 0, K // 64, K)
        assert s1.dtype == np.int64 and s2.dtype == np.int64 and s1.shape == (n,) and s2.shape == (n,)
        assert (_bits(_result(s1, K)) == _bits(fixed(t, K))).all(), (scene, kind, K)
        assert (s1 >= 0).all() and (s2 >= 0).all() and (s1[s2 > 0] > 0).all()
    assert s1.max() > 0


def test_sums_on_the_device_are_the_host_form():
    import torch
    t, n, _ = _scene("mesh")
    e = _emission(n)
    for host, dev in ((t.gatherFluxSums(1, 2, 256, cosinePower=8.0, numpy=True), t.gatherFluxSums(1, 2, 256, cosinePower=8.0)),
                      (t.gatherFluxSums(0, 2, 128, emission=e), t.gatherFluxSums(0, 2, 128, emission=torch.from_numpy(e).cuda())),
                      (t.gatherPathsSums(0, 2, 128, reflectivity=np.full(n, 0.7, np.float32)),
                       t.gatherPathsSums(0, 2, 128, reflectivity=torch.full((n,), 0.7, device="cuda")))):
        for h, d in zip(host, dev):
            assert isinstance(h, np.ndarray) and d.is_cuda and d.dtype == torch.int64
            assert (h == d.cpu().numpy()).all()


# ---------------------------------------------------------------------------------------------------------------
# 2. splits: of the chunks, of the range, of a chunk into work items
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", SCENES)
@pytest.mark.parametrize("kind", ["normal8", "emission", "specular", "diffuse"])
def test_sums_add_over_chunks_and_do_not_depend_on_the_range(scene, kind):
    t, n, _ = _scene(scene)
    _, sums, _, _ = _kind(kind, n)
    whole = sums(t, 0, 4, 256)
    head, tail = sums(t, 0, 1, 256), sums(t, 1, 3, 256)
    for k in range(2):
        assert (whole[k] == head[k] + tail[k]).all()
    assert (tail[0] != 0).any()
    # a split of the primitive range at an odd place; a range of five primitives is cut into 16 runs per chunk
    cut = n // 3 + 1
    a, b = sums(t, 1, 3, 256, primFirst=0, primCount=cut), sums(t, 1, 3, 256, primFirst=cut, primCount=n - cut)
    few = sums(t, 1, 3, 256, primFirst=cut - 2, primCount=5)
    for k in range(2):
        assert (np.concatenate([a[k], b[k]]) == tail[k]).all()
        assert (few[k] == tail[k][cut - 2:cut + 3]).all()
    # a chunk range that ends at the budget, and an empty one
    last = sums(t, 3, 1, 256)
    assert (last[0] == whole[0] - sums(t, 0, 3, 256)[0]).all()
    none = sums(t, 2, 0, 256)
    assert (none[0] == 0).all() and (none[1] == 0).all()


# ---------------------------------------------------------------------------------------------------------------
# 3. the squares
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", SCENES)
def test_unit_weights_square_to_the_sum_shifted(scene):
    """n = 1 without emission: every weight is 0 or 1, q = 2^40 and q2 = 2^28"""
    t, n, _ = _scene(scene)
    s1, s2 = t.gatherFluxSums(0, 4, 256, numpy=True)
    assert (s2 == s1 >> 12).all() and (s1 % (1 << 40) == 0).all() and (s1 > 0).any() and (s1 < 256 << 40).any()


@pytest.mark.parametrize("kind", ["specular", "diffuse"])
def test_path_squares_are_those_of_the_weights_the_debug_call_reports(kind):
    t, n, part = _scene("mesh")
    kw = dict(reflectivity=0.7, reflection=GR.SPECULAR if kind == "specular" else GR.DIFFUSE, maxBounces=16, cosinePower=8.0)
    s1, s2 = t.gatherPathsSums(0, 1, 64, numpy=True, **kw)
    prims = [int(np.flatnonzero(part == p)[k]) for p, k in ((cf.BOTTOM, 3), (cf.BOTTOM, 40), (cf.LEFT, 5), (cf.RIGHT, 77), (cf.TOP, 9))]
    distinct = set()
    for prim in prims:
        w = np.array([t.debugGatherPath(prim, k, **kw)["weight"] for k in range(64)], dtype=np.float32)
        distinct |= set(w.tolist())
        assert int(_np_q2(w, 65536.0).sum()) == int(s2[prim]), prim
        assert int(np.where(w > 0, np.floor(w.astype(np.float64) * 2.0 ** 40 + 0.5), 0).astype(np.int64).sum()) == int(s1[prim]), prim
    assert len(distinct) > 10  # (reflected weights: powers of 0.7 times g c^7, not a two-valued set)


@pytest.mark.parametrize("scene", SCENES)
@pytest.mark.parametrize("kind", ["normal1", "normal8", "specular", "diffuse"])
def test_sample_variance_is_bounded_by_the_mean(scene, kind):
    """0 <= w <= g for every NORMAL weight, so sum w^2 <= g sum w: m2 - m1^2 <= m1 (g - m1), up to the quantisation of
    the squares (half a unit of 2^-28 per sample in the mean) and of the weights (2^-41 g per sample): 2^-27 covers both"""
    t, n, _ = _scene(scene)
    _, sums, _, power = _kind(kind, n)
    D = 3 if scene == "mesh" else 2
    g = _g(power, D)
    s1, s2 = sums(t, 0, 4, 256)
    m1 = s1.astype(np.float64) / 2.0 ** 40 / 256
    m2 = s2.astype(np.float64) / 2.0 ** 28 / 256
    assert (m2 - m1 * m1 <= m1 * (g - m1) + 2.0 ** -27).all()
    assert (m1 <= g).all()


# ---------------------------------------------------------------------------------------------------------------
# 4. the adaptive call: identities
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,kind", [("mesh", "normal8"), ("disks2", "specular"), ("grid2", "emission"), ("mesh", "diffuse"),
                                        ("grid2", "source8")])
def test_target_zero_and_a_huge_target_are_the_fixed_k_calls(scene, kind):
    t, n, _ = _scene(scene)
    fixed, _, adaptive, _ = _kind(kind, n)
    flux, err, used, info = adaptive(t, 0.0, minSamples=64, maxSamples=512, returnInfo=True)
    assert (used == 512).all() and (_bits(flux) == _bits(fixed(t, 512))).all()
    assert info == {"rounds": 4, "unconverged": n, "totalSamples": 512 * n}
    flux, err, used, info = adaptive(t, 1e30, minSamples=128, maxSamples=512, returnInfo=True)
    assert (used == 128).all() and (_bits(flux) == _bits(fixed(t, 128))).all()
    assert info == {"rounds": 1, "unconverged": 0, "totalSamples": 128 * n}
    # min == max: one round, whatever the target
    flux, err, used, info = adaptive(t, 0.05, minSamples=192, maxSamples=192, returnInfo=True)
    assert (used == 192).all() and (_bits(flux) == _bits(fixed(t, 192))).all() and info["rounds"] == 1
    # an absolute target alone
    flux, err, used, info = adaptive(t, 0.0, absTarget=0.02, minSamples=64, maxSamples=1024, returnInfo=True)
    assert info["totalSamples"] == int(used.astype(np.int64).sum())
    assert (err[used < 1024] <= np.float32(0.02) * (1 + 1e-6)).all()


# ---------------------------------------------------------------------------------------------------------------
# 5. the adaptive call replayed: every decision is the numpy rule on the sums call's sums
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,kind", [("mesh", "normal8"), ("mesh", "specular"), ("grid2", "normal8"), ("disks2", "diffuse")])
def test_adaptive_replay(scene, kind):
    t, n, _ = _scene(scene)
    fixed, sums, adaptive, _ = _kind(kind, n)
    lo, hi, rel = 64, 1024, 0.05
    flux, err, used, info = adaptive(t, rel, minSamples=lo, maxSamples=hi, returnInfo=True)
    assert used.dtype == np.uint32 and flux.dtype == np.float32 and err.dtype == np.float32
    levels = [lo << r for r in range(5)]
    print(scene, kind, "samplesUsed:", dict(zip(*(a.tolist() for a in np.unique(used, return_counts=True)))), info)
    assert set(np.unique(used).tolist()) <= set(levels)
    if kind in ("specular", "diffuse"):  # (n = 1: the unoccluded top stops at once, the trench does not)
        assert len(np.unique(used)) >= 2
    assert info["totalSamples"] == int(used.astype(np.int64).sum())
    assert info["rounds"] == levels.index(int(used.max())) + 1
    at = {K: sums(t, 0, K // 64, hi) for K in levels}  # (wmax that of maxSamples, as in every round)
    for K in levels:
        here = used == K
        if not here.any():
            continue
        # no weight exceeds g: wmax cannot show, the flux is the fixed-K call's
        assert (_bits(flux[here]) == _bits(fixed(t, K)[here])).all(), K
        s1, s2 = at[K]
        assert (_bits(flux[here]) == _bits(_result(s1, K)[here])).all()
        _, se2 = np_moments(s1, s2, K)
        assert (_bits(err[here]) == _bits(np.sqrt(se2).astype(np.float32)[here])).all(), K
        if K > lo:  # it went on from K / 2 — and from every level before
            for J in levels[:levels.index(K)]:
                assert not np_converged(at[J][0], at[J][1], J, rel)[here].any(), (K, J)
        if K < hi:
            assert np_converged(s1, s2, K, rel)[here].all(), K
    top = used == hi
    assert info["unconverged"] == int((~np_converged(at[hi][0], at[hi][1], hi, rel))[top].sum())
    # tensors out without numpy=True: the same values
    if scene == "mesh":
        import torch
        kw = dict(cosinePower=8.0) if kind == "normal8" else dict(reflectivity=0.7, reflection=GR.SPECULAR, maxBounces=16)
        call = t.gatherFluxAdaptive if kind == "normal8" else t.gatherPathsAdaptive
        f2, e2, u2 = call(rel, minSamples=lo, maxSamples=hi, **kw)
        assert f2.is_cuda and e2.is_cuda and u2.is_cuda and u2.dtype == torch.int32
        assert (_bits(f2.cpu().numpy()) == _bits(flux)).all() and (_bits(e2.cpu().numpy()) == _bits(err)).all()
        assert (u2.cpu().numpy().astype(np.uint32) == used).all()


@pytest.mark.parametrize("scene,kind", [("mesh", "normal8"), ("grid2", "specular")])
def test_adaptive_over_a_split_range(scene, kind):
    t, n, _ = _scene(scene)
    _, _, adaptive, _ = _kind(kind, n)
    whole = adaptive(t, 0.05, minSamples=64, maxSamples=1024, returnInfo=True)
    cut = n // 3 + 1
    a = adaptive(t, 0.05, minSamples=64, maxSamples=1024, returnInfo=True, primFirst=0, primCount=cut)
    b = adaptive(t, 0.05, minSamples=64, maxSamples=1024, returnInfo=True, primFirst=cut, primCount=n - cut)
    for k in range(2):
        assert (_bits(np.concatenate([a[k], b[k]])) == _bits(whole[k])).all()
    assert (np.concatenate([a[2], b[2]]) == whole[2]).all()
    for key in ("unconverged", "totalSamples"):
        assert a[3][key] + b[3][key] == whole[3][key]
    assert max(a[3]["rounds"], b[3]["rounds"]) == whole[3]["rounds"]
    empty = adaptive(t, 0.05, returnInfo=True, primFirst=n, primCount=0)
    assert len(empty[0]) == 0 and empty[3] == {"rounds": 0, "unconverged": 0, "totalSamples": 0}


@pytest.mark.parametrize("kind", ["normal1", "specular"])  # (n = 1: the top stops at minSamples, the lists shrink block by block)
def test_a_list_of_several_decide_blocks(kind):
    """a 3-D disk cloud of some thousand primitives: the whole scene (leaf order, the next list from the blocks' counts
    in two passes), a range of more than one block (the caller's order) and ranges that fit one block give the same
    outputs; the flux is the fixed-K call's at every level"""
    t, n, _ = _scene("disks3")
    assert n > 3 * 1024
    fixed, sums, adaptive, _ = _kind(kind, n)
    s1, _ = sums(t, 0, 2, 128)
    assert (_bits(_result(s1, 128)) == _bits(fixed(t, 128))).all()
    whole = adaptive(t, 0.05, minSamples=64, maxSamples=512, returnInfo=True)
    flux, err, used, info = whole
    print(kind, "samplesUsed:", dict(zip(*(a.tolist() for a in np.unique(used, return_counts=True)))), info)
    assert info["totalSamples"] == int(used.astype(np.int64).sum()) and len(np.unique(used)) >= 2
    for K in np.unique(used).tolist():
        assert (_bits(flux[used == K]) == _bits(fixed(t, K)[used == K])).all(), K
    at = sums(t, 0, 8, 512)
    assert info["unconverged"] == int((~np_converged(at[0], at[1], 512, 0.05))[used == 512].sum())
    cuts = [0, 2500, 2500 + 700, n]  # more than two blocks, less than one, the rest
    parts = [adaptive(t, 0.05, minSamples=64, maxSamples=512, returnInfo=True, primFirst=a, primCount=b - a)
             for a, b in zip(cuts[:-1], cuts[1:])]
    for k in range(3):
        assert (np.concatenate([p[k] for p in parts]).view(np.uint32) == whole[k].view(np.uint32)).all(), k
    assert sum(p[3]["unconverged"] for p in parts) == info["unconverged"]


# ---------------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------------
def _spec(**kw):
    s = capi.GatherSpecPOD(cosinePower=1.0, mode=0, paths=0, reflection=0, maxBounces=16, reflectivityScalar=0.7)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def test_refusals_leave_the_outputs_untouched_and_the_context_usable():
    t, n, _ = _scene("mesh")
    L = t._L
    fp, u32p, i64p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_int64)
    want = t.gatherFluxAdaptive(0.05, minSamples=64, maxSamples=256, numpy=True)
    table = np.full(n, 0.5, np.float32)
    nan = float("nan")

    def adaptive(spec, lo, hi, rel, ab, first=0, count=n):
        flux, err = np.full(n, POISON, np.float32), np.full(n, POISON, np.float32)
        used = np.full(n, 0xDEAD, np.uint32)
        info = capi.GatherAdaptiveInfoPOD(rounds=77, unconverged=77, totalSamples=77)
        rc = L.vr_gather_adaptive(t._h, C.byref(spec) if spec is not None else None, first, count, lo, hi, rel, ab,
                                  flux.ctypes.data_as(fp), err.ctypes.data_as(fp), used.ctypes.data_as(u32p), C.byref(info))
        untouched = (flux == POISON).all() and (err == POISON).all() and (used == 0xDEAD).all() and info.rounds == 77
        return rc, untouched

    def sums(spec, c0, c, budget, first=0, count=n):
        s1, s2 = np.full(n, -5, np.int64), np.full(n, -5, np.int64)
        rc = L.vr_gather_sums(t._h, C.byref(spec), first, count, c0, c, budget, s1.ctypes.data_as(i64p), s2.ctypes.data_as(i64p))
        return rc, (s1 == -5).all() and (s2 == -5).all()

    paths_with_emission = _spec(paths=1, emission=table.ctypes.data)
    cases = [adaptive(_spec(), 96, 192, 0.05, 0.0),           # minSamples no multiple of 64
             adaptive(_spec(), 0, 0, 0.05, 0.0),
             adaptive(_spec(), 64, 192, 0.05, 0.0),           # maxSamples = 3 x min
             adaptive(_spec(), 128, 64, 0.05, 0.0),
             adaptive(_spec(), 64, 256, nan, 0.0), adaptive(_spec(), 64, 256, 0.05, nan),
             adaptive(_spec(), 64, 256, -0.05, 0.0), adaptive(_spec(), 64, 256, 0.05, -1.0),
             adaptive(paths_with_emission, 64, 256, 0.05, 0.0),   # paths with an emission table
             adaptive(_spec(paths=1, mode=1, cosinePower=8.0), 64, 256, 0.05, 0.0),
             adaptive(_spec(paths=2), 64, 256, 0.05, 0.0),
             adaptive(_spec(paths=1, reflectivityScalar=1.5), 64, 256, 0.05, 0.0),
             adaptive(_spec(paths=1, reflection=2), 64, 256, 0.05, 0.0),
             adaptive(_spec(mode=1), 64, 256, 0.05, 0.0),          # SOURCE at cosinePower 1
             adaptive(_spec(cosinePower=8.0), 1 << 20, 1 << 20, 0.05, 0.0),  # maxSamples x g beyond 2^22
             adaptive(_spec(), 64, 256, 0.05, 0.0, first=1),       # the range ends beyond the scene
             adaptive(None, 64, 256, 0.05, 0.0),
             sums(_spec(), 3, 2, 256),                             # chunks beyond the budget
             sums(_spec(), 0, 1, 63), sums(_spec(), 0, 1, 0),
             sums(paths_with_emission, 0, 1, 64), sums(_spec(paths=2), 0, 1, 64), sums(_spec(), 0, 1, 64, first=n, count=1)]
    for k, (rc, untouched) in enumerate(cases):
        assert rc == capi.VR_E_INVALID and untouched and L.vr_last_error(t._h), k
    # a bad table entry is named; nothing is written
    bad = table.copy()
    bad[17] = -0.25
    rc, untouched = adaptive(_spec(paths=1, reflectivity=bad.ctypes.data), 64, 256, 0.05, 0.0)
    assert rc == capi.VR_E_INVALID and untouched and b"reflectivity[17]" in L.vr_last_error(t._h)
    # the device forms refuse host memory
    import torch
    dev = torch.full((n,), float(POISON), device="cuda")
    host = np.full(n, POISON, np.float32)
    info = capi.GatherAdaptiveInfoPOD()
    assert L.vr_gather_adaptive_device(t._h, C.byref(_spec()), 0, n, 64, 256, 0.05, 0.0, C.c_void_p(host.ctypes.data), None, None,
                                       C.byref(info), None) == capi.VR_E_INVALID
    assert L.vr_gather_adaptive_device(t._h, C.byref(_spec(emission=table.ctypes.data)), 0, n, 64, 256, 0.05, 0.0,
                                       C.c_void_p(dev.data_ptr()), None, None, C.byref(info), None) == capi.VR_E_INVALID
    s1 = torch.full((n,), -5, dtype=torch.int64, device="cuda")
    h2 = np.full(n, -5, np.int64)
    assert L.vr_gather_sums_device(t._h, C.byref(_spec()), 0, n, 0, 1, 64, C.c_void_p(s1.data_ptr()), C.c_void_p(h2.ctypes.data),
                                   None) == capi.VR_E_INVALID
    torch.cuda.synchronize()
    assert (host == POISON).all() and bool((dev == float(POISON)).all()) and bool((s1 == -5).all()) and (h2 == -5).all()
    # stdErr and samplesUsed may be NULL; nothing to do is VR_OK after the checks
    flux = np.full(n, POISON, np.float32)
    assert L.vr_gather_adaptive(t._h, C.byref(_spec()), 0, n, 64, 256, 0.05, 0.0, flux.ctypes.data_as(fp), None, None,
                                C.byref(info)) == capi.VR_OK
    assert (_bits(flux) == _bits(want[0])).all()
    assert L.vr_gather_adaptive(t._h, C.byref(_spec()), 0, 0, 64, 256, 0.05, 0.0, None, None, None, C.byref(info)) == capi.VR_OK
    with pytest.raises(vr.VrError, match="multiple of 64"):
        t.gatherFluxAdaptive(0.05, minSamples=96, maxSamples=192)
    with pytest.raises(vr.VrError, match="power of two"):
        t.gatherPathsAdaptive(0.05, reflectivity=0.7, minSamples=64, maxSamples=192)
    with pytest.raises(vr.VrError, match="beyond the budget"):
        t.gatherFluxSums(3, 2, 256)
    with pytest.raises(ValueError):
        t.gatherPathsAdaptive(0.05)
    # ... and the context still answers
    again = t.gatherFluxAdaptive(0.05, minSamples=64, maxSamples=256, numpy=True)
    for a, b in zip(again, want):
        assert (a.view(np.uint32) == b.view(np.uint32)).all()


def test_an_adaptive_gather_needs_what_a_prepare_left():
    g = cf.trench_mesh()
    t = _mesh_tracer(g)
    t.setParticleType(vr.DiffuseParticle(1.0, "flux"))
    t.setNumberOfRaysFixed(1000)
    t.setRngSeed(SEED)
    with pytest.raises(vr.VrError, match="nothing to gather from"):
        t.gatherFluxAdaptive(0.05, numpy=True)
    with pytest.raises(vr.VrError, match="nothing to gather from"):
        t.gatherPathsSums(0, 1, 64, reflectivity=0.7)
    t.applyPrepare()
    want = _scene("mesh")[0].gatherFluxAdaptive(0.05, maxSamples=256, numpy=True)
    got = t.gatherFluxAdaptive(0.05, maxSamples=256, numpy=True)
    assert (_bits(got[0]) == _bits(want[0])).all() and (got[2] == want[2]).all()


# ---------------------------------------------------------------------------------------------------------------
# 7. where the work goes
# ---------------------------------------------------------------------------------------------------------------
def test_work_goes_where_the_variance_is():
    """n = 1 on the trench: a top primitive sees the whole source, every weight is 1 and the error is exactly 0 at
    minSamples; walls and bottom see part of it and go on"""
    t, n, part = _scene("mesh")
    flux, err, used = t.gatherFluxAdaptive(0.05, minSamples=64, maxSamples=1024, numpy=True)
    top = part == cf.TOP
    assert (used[top] == 64).all() and (err[top] == 0).all() and (flux[top] == 1).all()
    assert (used[~top] > 64).any() and (err[~top] > 0).any()
    assert used[~top].astype(np.int64).sum() > 4 * 64 * int((~top).sum())  # (most of them, several doublings)


# ---------------------------------------------------------------------------------------------------------------
# 8. the error is calibrated
# ---------------------------------------------------------------------------------------------------------------
def test_reported_error_is_the_variance_over_seeds():
    """16 seeds (multiples of 1000: seed S and S + 1 share chunk engines, the engine's seed being a hash of S + chunk),
    K = 256, the primitives with 0.05 < F < 0.95: sum of the mean reported se2 over sum of the variance of F over seeds.
    15 degrees of freedom and 200 primitives or more: the ratio's standard deviation is about sqrt(2 / 15 / 200) = 2.6 %"""
    g = cf.trench_mesh()
    t = _prepared(_mesh_tracer(g))
    F, E = [], []
    for s in range(16):
        t.setRngSeed(1000 * (s + 1))
        s1, s2 = t.gatherFluxSums(0, 4, 256, numpy=True)
        m1, se2 = np_moments(s1, s2, 256)
        F.append(m1)
        E.append(se2)
    F, E = np.array(F), np.array(E)
    mid = (F.mean(0) > 0.05) & (F.mean(0) < 0.95)
    assert mid.sum() >= 200, mid.sum()
    ratio = E.mean(0)[mid].sum() / F.var(0, ddof=1)[mid].sum()
    print("calibration: %d primitives, sum mean se2 / sum var F = %.4f" % (mid.sum(), ratio))
    assert 0.85 <= ratio <= 1.15, ratio


# ---------------------------------------------------------------------------------------------------------------
# 9. an apply is untouched
# ---------------------------------------------------------------------------------------------------------------
def _apply_twice(between):
    g = cf.trench_mesh()
    t = _mesh_tracer(g)
    t.setParticleType(vr.DiffuseParticle(0.3, "flux"))
    t.setNumberOfRaysFixed(200_000)
    t.setRngSeed(SEED)
    t.setUseRandomSeeds(False)
    t.apply()
    first = np.array(t.getLocalData().getVectorData("flux"))
    if between:
        t.gatherFluxAdaptive(0.05, maxSamples=512, numpy=True)
        t.gatherPathsAdaptive(0.05, sticking=np.full(len(g.tris), 0.2, np.float32), reflection=GR.DIFFUSE, cosinePower=8.0, maxSamples=256)
        t.gatherFluxSums(1, 2, 256)
        assert (_bits(t.getLocalData().getVectorData("flux")) == _bits(first)).all()
    t.apply()
    return first, np.array(t.getLocalData().getVectorData("flux")), t.getRayTraceInfo().as_dict()


def test_an_apply_is_untouched_by_an_adaptive_gather():
    f0, s0, i0 = _apply_twice(False)
    f1, s1, i1 = _apply_twice(True)
    assert (_bits(f0) == _bits(f1)).all() and (_bits(s0) == _bits(s1)).all()
    skip = {"time", "timeBuild", "timeTrace", "timeTraceKernel", "timeGenKernel"}
    assert {k: v for k, v in i0.items() if k not in skip} == {k: v for k, v in i1.items() if k not in skip}


# ---------------------------------------------------------------------------------------------------------------
# 10. the C++ façade
# ---------------------------------------------------------------------------------------------------------------
def test_cpp_facade_gather_adaptive(tmp_path):
    flags = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include",
             "-I", os.path.join(ROOT, "include", "viennaray_amd"), "-I", os.path.join(ROOT, "include")]
    src = os.path.join(ROOT, "tests", "aux", "facade_gather_adaptive.cpp")
    exe = tmp_path / "facade_gather_adaptive"
    lib = os.path.join(ROOT, "viennaray_amd")
    subprocess.check_call(["g++", "-O1"] + flags + [src, "-o", str(exe), "-L", lib, "-lviennaray_amd",
                                                    "-L", "/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib,
                                                    "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "facade gather adaptive ok" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
