"""solveRadiosity on the device (vr_radiosity_links_device, vr_radiosity_solve*, vr_radiosity_direct_device,
vr_debug_radiosity_links; Trace.solveRadiosity): the steady-state flux of a diffusely re-emitting species from a recorded
link table.  An iteration from links is by definition the int64 sum gatherFlux with an emission table computes, so the
solve is pinned bit for bit against chained gatherFlux calls; the links against castRays; exact values on a flat plane;
the fixed point against the closed form of tests/closed_forms.py with a bound derived from the one-iteration bound of
test_gather_flux.test_radiosity_fixed_point; reuse, staleness, refusals and the C++ façade."""
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
SEED = 7
ONE = np.float32(1.0)
MESH_BCS = [BC.REFLECTIVE_BOUNDARY, BC.PERIODIC_BOUNDARY, BC.REFLECTIVE_BOUNDARY]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _prepared(t, seed=SEED):
    t.setParticleType(vr.DiffuseParticle(1.0, "flux"))
    t.setNumberOfRaysFixed(1000)
    t.setRngSeed(seed)
    t.applyPrepare()
    return t


def _new_mesh(seed=SEED):
    g = cf.trench_mesh()
    t = vr.TraceTriangle(3)
    t.setGeometry(g.verts, g.tris, 1.0)
    t.setBoundaryConditions(MESH_BCS)
    return _prepared(t, seed), g


@functools.lru_cache(maxsize=None)
def _mesh():
    t, g = _new_mesh()
    cen, _ = cf.triangle_centroids(g)
    coord = np.where(g.part == cf.BOTTOM, cen[:, 0], cen[:, 2])  # x on the bottom, z on the walls (unused on the top)
    return t, g, coord


@functools.lru_cache(maxsize=None)
def _disks2():
    g = cf.trench_disks(2)
    assert len(g.points) % 64 != 0
    t = vr.TraceDisk(2)
    t.setGeometry(g.points, g.normals, 1.0)
    t.setBoundaryConditions([BC.REFLECTIVE_BOUNDARY, BC.REFLECTIVE_BOUNDARY])
    t.setSourceDirection(cf.POS_Y)
    return _prepared(t), g


@functools.lru_cache(maxsize=None)
def _flat(flipped=False):
    n = 16
    i, j = np.meshgrid(np.arange(n, dtype=np.float32), np.arange(n, dtype=np.float32), indexing="ij")
    pts = np.stack([i.ravel(), j.ravel(), np.zeros(n * n, np.float32)], 1)
    nrm = np.tile(np.array([0, 0, 1], np.float32), (n * n, 1))
    t = vr.TraceDisk(3)
    t.setGeometry(pts, nrm, 1.0)
    t.setBoundaryConditions([BC.PERIODIC_BOUNDARY] * 3)
    if flipped:
        t.setSourceDirection(vr.TraceDirection.NEG_Z)
    return _prepared(t)


def _scene(name):
    return _mesh()[:2] if name == "mesh" else _disks2()


def _rho_table(g):
    """a per-primitive reflectivity with zeros on one part (the bottom) and different values elsewhere"""
    n = len(g.part)
    rho = (0.3 + 0.6 * (np.arange(n) % 7) / 6.0).astype(np.float32)
    rho[g.part == cf.BOTTOM] = 0.0
    return rho


# ---------------------------------------------------------------------------------------------------------------
# 1. the same bits as the gather
# ---------------------------------------------------------------------------------------------------------------
def _chain(t, K, rho, steps, power=1.0):
    """F_0 .. F_steps by chaining the existing call: F_t = gatherFlux(K, emission=(rho F_{t-1}).astype(float32))"""
    F = [t.gatherFlux(K, cosinePower=power, numpy=True)]
    for _ in range(steps):
        F.append(t.gatherFlux(K, cosinePower=power, emission=(rho * F[-1]).astype(np.float32)))
    return F


@pytest.mark.parametrize("K", [64, 100, 4096])
@pytest.mark.parametrize("scene", ["mesh", "disks2"])
def test_same_bits_as_chained_gathers(scene, K):
    t, g = _scene(scene)
    rho = _rho_table(g)
    ref = _chain(t, K, rho, 3)
    out, its, res = t.solveRadiosity(K, reflectivity=rho, maxIterations=0, returnInfo=True)
    assert out.dtype == np.float32 and out.shape == ref[0].shape and (its, res) == (0, 0.0)
    assert (_bits(out) == _bits(ref[0])).all()
    for step in (1, 2, 3):
        out, its, res = t.solveRadiosity(K, reflectivity=rho, tolerance=0.0, maxIterations=step, returnInfo=True)
        assert its == step
        assert (_bits(out) == _bits(ref[step])).all(), (step, np.nonzero(_bits(out) != _bits(ref[step]))[0][:8])
        assert np.float32(res) == np.abs(ref[step] - ref[step - 1]).max()
    assert (ref[3] >= ref[0]).all() and (ref[3] > ref[0]).any()  # (the table brings something back: the links are not all -1)


def test_same_bits_with_a_power_cosine_source_and_a_tensor():
    import torch
    t, g, _ = _mesh()
    rho = _rho_table(g)
    ref = _chain(t, 100, rho, 2, power=8.0)
    out = t.solveRadiosity(100, reflectivity=rho, cosinePower=8.0, tolerance=0.0, maxIterations=2)
    assert (_bits(out) == _bits(ref[2])).all()
    dev = t.solveRadiosity(100, reflectivity=torch.from_numpy(rho).cuda(), cosinePower=8.0, tolerance=0.0, maxIterations=2)
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and (_bits(dev.cpu().numpy()) == _bits(ref[2])).all()
    stick = t.solveRadiosity(100, sticking=torch.from_numpy((ONE - rho).astype(np.float32)).cuda(), cosinePower=8.0, tolerance=0.0,
                             maxIterations=2)
    assert (_bits(stick.cpu().numpy()) == _bits(t.solveRadiosity(100, sticking=(ONE - rho).astype(np.float32), cosinePower=8.0,
                                                                   tolerance=0.0, maxIterations=2))).all()
    # F_0 straight from the table
    d = torch.empty(len(rho), dtype=torch.float32, device="cuda")
    assert t._L.vr_radiosity_direct_device(t._h, C.c_void_p(d.data_ptr()), None) == capi.VR_OK
    torch.cuda.synchronize()
    assert (_bits(d.cpu().numpy()) == _bits(ref[0])).all()


def test_batching_cannot_show():
    """the stopping iteration found through batches of launches is the one a loop of single iterations finds"""
    t, g, _ = _mesh()
    full, its, res = t.solveRadiosity(64, sticking=0.3, tolerance=1e-3, returnInfo=True)
    assert 3 < its < 100 and 0 < res <= 1e-3
    one_more = t.solveRadiosity(64, sticking=0.3, tolerance=0.0, maxIterations=its + 1)
    for k in range(1, its + 1):
        out, t_k, r_k = t.solveRadiosity(64, sticking=0.3, tolerance=0.0, maxIterations=k, returnInfo=True)
        assert t_k == k and (r_k > 1e-3) == (k < its), (k, r_k)
    assert (_bits(out) == _bits(full)).all() and r_k == res
    assert (_bits(one_more) != _bits(full)).any()  # (an overshoot would have shown)


# ---------------------------------------------------------------------------------------------------------------
# 2. the links reproduce through a cast
# ---------------------------------------------------------------------------------------------------------------
def test_links_match_a_cast_of_the_gathers_samples():
    t, g, _ = _mesh()
    K = 256
    t.radiosityLinks(K)
    cen, nrm = cf.triangle_centroids(g)
    nrm = nrm / np.linalg.norm(nrm, axis=1)[:, None]
    seen = set()
    for part, k in ((cf.BOTTOM, 3), (cf.LEFT, 11), (cf.TOP, 5)):
        prim = int(np.nonzero(g.part == part)[0][k])
        o, _, d = t.debugGatherSamples(prim, 0, K)
        hit, _ = t.castRays(np.tile(o, (K, 1)), d, followBoundaries=True)
        # the front-side rule: a geometry hit whose direction AT THE HIT opposes the normal of the primitive hit.  Here
        # that direction is the initial one: the y walls wrap, which changes no direction, and a sample that reaches a
        # reflective x wall (|x| = L) has left the trench upwards and keeps rising, so it meets no geometry afterwards
        want = np.full(K, -1, np.int32)
        geo = hit >= 0
        dn = np.einsum("ij,ij->i", d[geo].astype(np.float64), nrm[hit[geo]])
        assert (np.abs(dn) > 1e-6).all()
        want[geo] = np.where(dn < 0, hit[geo], -1)
        got = t.debugRadiosityLinks(prim, 0, K)
        assert got.dtype == np.int32 and (got == want).all(), (prim, np.nonzero(got != want)[0][:8])
        # a run from the middle, and the last sample
        assert (t.debugRadiosityLinks(prim, 100, 60) == got[100:160]).all() and t.debugRadiosityLinks(prim, K - 1, 1)[0] == got[-1]
        seen.add(bool((got >= 0).any()))
    assert seen == {True, False}  # (the top sees no surface, the bottom and the wall do)


# ---------------------------------------------------------------------------------------------------------------
# 3. exact values
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rho", [0.0, 0.5, 0.99, 1.0])
def test_flat_plane_is_exactly_one_whatever_the_reflectivity(rho):
    out, its, res = _flat().solveRadiosity(64, reflectivity=rho, returnInfo=True)
    assert out.shape == (256,) and (_bits(out) == _bits(ONE)).all() and (its, res) == (1, 0.0)
    assert (_flat().debugRadiosityLinks(17, 0, 64) == -1).all()


def test_flat_plane_facing_away_is_zero():
    out, its, res = _flat(True).solveRadiosity(64, sticking=0.1, returnInfo=True)
    assert (_bits(out) == 0).all() and (its, res) == (1, 0.0)


# ---------------------------------------------------------------------------------------------------------------
# 4. the closed form
# ---------------------------------------------------------------------------------------------------------------
def _bd(F, g, k):
    """5 sigma of a mean of k samples in [0, g] with expectation F (Bhatia-Davis: var <= F (g - F)); test_gather_flux._bd"""
    F = np.asarray(F, dtype=np.float64)
    return 5.0 * np.sqrt(np.clip(F * (g - F), 0.0, None) / k) + 1e-5


def test_fixed_point_against_the_closed_form():
    """Mesh, s = 0.5, K = 16384, tolerance 1e-6.  The solve's error is (I - Khat rho)^-1 applied to the one-iteration
    error at the fixed point, which test_gather_flux.test_radiosity_fixed_point bounds per primitive by _bd(F_i, M, K) +
    REFERENCE_ERROR; the stopping rule adds at most tolerance to it.  Every row of Khat sums to at most 1, so the inverse's
    infinity norm is at most 1 / (1 - rho): bound = (max_i [_bd + REFERENCE_ERROR] + tolerance) / (1 - rho)."""
    s, K, tol = 0.5, 16384, 1e-6
    t, g, coord = _mesh()
    R = cf.radiosity(s=s)
    F = np.ones(len(g.tris))
    for p in (cf.BOTTOM, cf.LEFT, cf.RIGHT):
        sel, seg = g.part == p, R.part == p
        mid = 0.5 * (R.lo[seg] + R.hi[seg])
        order = np.argsort(mid)
        F[sel] = np.interp(coord[sel], mid[order], R.F[seg][order])
    top = g.part == cf.TOP
    rho = np.where(top, 0.0, 1.0 - s).astype(np.float32)  # (R's convention: the flat top re-emits nothing that comes back)
    out, its, res = t.solveRadiosity(K, reflectivity=rho, tolerance=tol, returnInfo=True)
    t.freeRadiosityLinks()  # (42 MB: not kept for the rest of the module)
    assert 1 <= its < 1000 and res <= tol
    assert (_bits(out[top]) == _bits(ONE)).all()
    M = max(1.0, float(((1 - s) * F[~top]).max()))
    bound = (float((_bd(F[~top], M, K) + cf.REFERENCE_ERROR).max()) + tol) / (1.0 - (1.0 - s))
    err = np.abs(out[~top].astype(np.float64) - F[~top])
    k = int(np.argmax(err))
    print("radiosity solve s=%.1f K=%d: %d iterations, residual %.2e; worst primitive uses %.0f %% of the bound %.5f "
          "(got %.5f ref %.5f)" % (s, K, its, res, 100 * err[k] / bound, bound, out[~top][k], F[~top][k]))
    assert (err <= bound).all(), [(int(q), float(out[~top][q]), float(F[~top][q])) for q in np.nonzero(err > bound)[0][:10]]


# ---------------------------------------------------------------------------------------------------------------
# 5. properties
# ---------------------------------------------------------------------------------------------------------------
def test_iterates_grow_and_stay_below_the_geometric_bound():
    t, g = _disks2()
    rho = _rho_table(g)
    rho_max = float(rho.max())
    prev = t.solveRadiosity(128, reflectivity=rho, maxIterations=0)
    for k in range(1, 6):
        out = t.solveRadiosity(128, reflectivity=rho, tolerance=0.0, maxIterations=k)
        assert (out >= prev).all(), k
        prev = out
    final = t.solveRadiosity(128, reflectivity=rho, tolerance=1e-6)
    g_n = 1.0  # g_D(1)
    assert (final >= prev).all() and float(final.max()) <= g_n / (1.0 - rho_max) * (1 + 1e-6)


# ---------------------------------------------------------------------------------------------------------------
# 6. reuse and state
# ---------------------------------------------------------------------------------------------------------------
def test_two_species_share_one_table():
    t, g = _new_mesh()
    a = t.solveRadiosity(64, sticking=0.1)
    assert t._L.vr_radiosity_resident(t._h, 64, 1.0) == 1 and t._L.vr_radiosity_resident(t._h, 128, 1.0) == 0
    builds = []
    real = t.radiosityLinks
    t.radiosityLinks = lambda *args, **kw: (builds.append(args), real(*args, **kw))
    b = t.solveRadiosity(64, sticking=0.5)
    assert builds == []  # reused
    fresh_a, fresh_b = _new_mesh()[0].solveRadiosity(64, sticking=0.1), _new_mesh()[0].solveRadiosity(64, sticking=0.5)
    assert (_bits(a) == _bits(fresh_a)).all() and (_bits(b) == _bits(fresh_b)).all() and (_bits(a) != _bits(b)).any()
    t.solveRadiosity(128, sticking=0.5)
    assert len(builds) == 1 and t.radiosityLinkBytes(128) == 640 * 128 * 4 + 640 * 8


def _raw_solve(t, rho, scalar, tol, its, out):
    fp = C.POINTER(C.c_float)
    n_it, res = C.c_uint32(0), C.c_float(0)
    return t._L.vr_radiosity_solve(t._h, rho.ctypes.data_as(fp) if rho is not None else None, scalar, tol, its,
                                   out.ctypes.data_as(fp) if out is not None else None, C.byref(n_it), C.byref(res))


def test_a_stale_table_is_refused_with_the_reason_and_python_rebuilds():
    t, g = _new_mesh()
    n = len(g.tris)
    want = t.solveRadiosity(64, sticking=0.2)
    poison = np.float32(-123.5)

    def refused(reason):
        out = np.full(n, poison, np.float32)
        assert _raw_solve(t, None, 0.8, 1e-4, 1000, out) == capi.VR_E_STATE and (out == poison).all()
        msg = t._L.vr_last_error(t._h).decode()
        assert "no longer matches" in msg and reason in msg, msg
        links = np.zeros(4, np.int32)
        assert t._L.vr_debug_radiosity_links(t._h, 0, 0, 4, links.ctypes.data_as(C.POINTER(C.c_int32))) == capi.VR_E_STATE

    t.setRngSeed(SEED + 1)
    refused("seed")
    other = t.solveRadiosity(64, sticking=0.2)  # the Python call rebuilds
    assert (_bits(other) != _bits(want)).any()
    t.setRngSeed(SEED)
    refused("seed")
    assert (_bits(t.solveRadiosity(64, sticking=0.2)) == _bits(want)).all()

    t.setBoundaryConditions([BC.REFLECTIVE_BOUNDARY, BC.REFLECTIVE_BOUNDARY, BC.REFLECTIVE_BOUNDARY])
    refused("boundary conditions")
    with pytest.raises(vr.VrError, match="nothing to gather from"):  # (the rebuild needs a prepare for the new walls)
        t.solveRadiosity(64, sticking=0.2)
    t.applyPrepare()
    refused("boundary conditions")
    t.solveRadiosity(64, sticking=0.2)
    t.setBoundaryConditions(MESH_BCS)
    t.applyPrepare()
    assert (_bits(t.solveRadiosity(64, sticking=0.2)) == _bits(want)).all()

    t.setMaxBoundaryHits(3)
    refused("maxBoundaryHits")
    t.setMaxBoundaryHits(1000)
    assert _raw_solve(t, None, 0.8, 1e-4, 1000, np.empty(n, np.float32)) == capi.VR_OK

    t.setGeometry(g.verts, g.tris[:-2], 1.0)  # a new geometry
    out = np.full(n - 2, poison, np.float32)
    assert _raw_solve(t, None, 0.8, 1e-4, 1000, out) == capi.VR_E_STATE and (out == poison).all()
    assert "geometry" in t._L.vr_last_error(t._h).decode()
    t.applyPrepare()
    assert _raw_solve(t, None, 0.8, 1e-4, 1000, out) == capi.VR_E_STATE and "geometry" in t._L.vr_last_error(t._h).decode()
    assert t.solveRadiosity(64, sticking=0.2).shape == (n - 2,)


def _apply_twice(solve_between):
    g = cf.trench_mesh()
    t = vr.TraceTriangle(3)
    t.setGeometry(g.verts, g.tris, 1.0)
    t.setBoundaryConditions(MESH_BCS)
    t.setParticleType(vr.DiffuseParticle(0.3, "flux"))
    t.setNumberOfRaysFixed(200_000)
    t.setRngSeed(SEED)
    t.setUseRandomSeeds(False)
    t.apply()
    first = np.array(t.getLocalData().getVectorData("flux"))
    if solve_between:
        t.radiosityLinks(128)
        t.solveRadiosity(128, sticking=0.3)
        assert (_bits(t.getLocalData().getVectorData("flux")) == _bits(first)).all()
    t.apply()
    return first, np.array(t.getLocalData().getVectorData("flux")), t.getRayTraceInfo().as_dict()


def test_an_apply_is_untouched_by_a_link_build_and_a_solve():
    f0, s0, i0 = _apply_twice(False)
    f1, s1, i1 = _apply_twice(True)
    assert (_bits(f0) == _bits(f1)).all() and (_bits(s0) == _bits(s1)).all()
    skip = {"time", "timeBuild", "timeTrace", "timeTraceKernel", "timeGenKernel"}
    assert {k: v for k, v in i0.items() if k not in skip} == {k: v for k, v in i1.items() if k not in skip}


# ---------------------------------------------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_out_untouched_and_the_context_usable():
    import torch
    t, g = _new_mesh()
    n = len(g.tris)
    L = t._L
    poison = np.float32(-123.5)
    want = t.solveRadiosity(64, sticking=0.5)

    def err():
        return L.vr_last_error(t._h).decode()

    out = np.full(n, poison, np.float32)
    rho = np.full(n, 0.5, np.float32)
    rho[5], rho[9] = np.nan, np.nan
    assert _raw_solve(t, rho, 0.0, 1e-4, 1000, out) == capi.VR_E_INVALID and (out == poison).all()
    assert "reflectivity[5]" in err(), err()
    rho = np.full(n, 0.5, np.float32)
    rho[n - 1] = 1.5
    assert _raw_solve(t, rho, 0.0, 1e-4, 1000, out) == capi.VR_E_INVALID and (out == poison).all() and "[%d]" % (n - 1) in err()
    rho[n - 1], rho[7] = 0.5, -1e-3
    assert _raw_solve(t, rho, 0.0, 1e-4, 1000, out) == capi.VR_E_INVALID and (out == poison).all() and "[7]" in err()
    for scalar in (1.5, -0.25, float("nan")):
        assert _raw_solve(t, None, scalar, 1e-4, 1000, out) == capi.VR_E_INVALID and (out == poison).all()
    for tol in (-1e-6, float("nan")):
        assert _raw_solve(t, None, 0.5, tol, 1000, out) == capi.VR_E_INVALID and (out == poison).all() and "tolerance" in err()
    assert _raw_solve(t, None, 0.5, 1e-4, 1000, None) == capi.VR_E_INVALID
    # the device form refuses host memory, for either pointer
    dev = torch.full((n,), float(poison), device="cuda")
    good = np.full(n, 0.5, np.float32)
    its, res = C.c_uint32(0), C.c_float(0)
    assert L.vr_radiosity_solve_device(t._h, None, 0.5, 1e-4, 1000, C.c_void_p(out.ctypes.data), C.byref(its), C.byref(res),
                                       None) == capi.VR_E_INVALID
    assert L.vr_radiosity_solve_device(t._h, C.c_void_p(good.ctypes.data), 0.0, 1e-4, 1000, C.c_void_p(dev.data_ptr()), C.byref(its),
                                       C.byref(res), None) == capi.VR_E_INVALID
    # a NaN in a device table
    bad = torch.full((n,), 0.5, device="cuda")
    bad[5] = float("nan")
    assert L.vr_radiosity_solve_device(t._h, C.c_void_p(bad.data_ptr()), 0.0, 1e-4, 1000, C.c_void_p(dev.data_ptr()), C.byref(its),
                                       C.byref(res), None) == capi.VR_E_INVALID and "reflectivity[5]" in err()
    torch.cuda.synchronize()
    assert (out == poison).all() and bool((dev == float(poison)).all())
    with pytest.raises(ValueError):
        t.solveRadiosity(64, sticking=torch.zeros(n, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        t.solveRadiosity(64)
    with pytest.raises(ValueError):
        t.solveRadiosity(64, sticking=0.5, reflectivity=0.5)
    # the link build refuses what the gather refuses
    for samples, power in ((0, 1.0), (64, 0.5), (64, float("nan")), ((1 << 22) + 1, 1.0)):
        assert L.vr_radiosity_links_device(t._h, samples, power, None) == capi.VR_E_INVALID, (samples, power)
    # the timing entry point: a table, a reflectivity in [0, 1], a count
    ms = C.c_float(-1.0)
    assert L.vr_debug_radiosity_time_iterations(t._h, 0.5, 4, 1, C.byref(ms)) == capi.VR_OK and ms.value > 0
    assert L.vr_debug_radiosity_time_iterations(t._h, 0.5, 4, 0, C.byref(ms)) == capi.VR_OK and ms.value > 0
    assert L.vr_debug_radiosity_time_iterations(t._h, 1.5, 4, 1, C.byref(ms)) == capi.VR_E_INVALID
    assert L.vr_debug_radiosity_time_iterations(t._h, 0.5, 0, 1, C.byref(ms)) == capi.VR_E_INVALID
    # ... and after all that the table is still there and answers
    assert _raw_solve(t, None, 0.5, 1e-4, 1000, out) == capi.VR_OK and (_bits(out) == _bits(want)).all()
    # no table: VR_E_STATE
    t.freeRadiosityLinks()
    out = np.full(n, poison, np.float32)
    assert _raw_solve(t, None, 0.5, 1e-4, 1000, out) == capi.VR_E_STATE and (out == poison).all() and "no link table" in err()
    assert L.vr_radiosity_direct_device(t._h, C.c_void_p(dev.data_ptr()), None) == capi.VR_E_STATE
    fresh = vr.TraceTriangle(3)
    fresh.setGeometry(g.verts, g.tris, 1.0)
    assert _raw_solve(fresh, None, 0.5, 1e-4, 1000, out) == capi.VR_E_STATE and (out == poison).all()
    assert fresh._L.vr_radiosity_links_device(fresh._h, 64, 1.0, None) == capi.VR_E_STATE  # nothing prepared
    assert (_bits(t.solveRadiosity(64, sticking=0.5)) == _bits(want)).all()


# ---------------------------------------------------------------------------------------------------------------
# 8. the C++ façade
# ---------------------------------------------------------------------------------------------------------------
def test_cpp_facade_radiosity(tmp_path):
    """tests/aux/facade_radiosity.cpp on the 3-D trench disks: its checks hold, and the flux it prints bit-equals the Python call"""
    g = cf.trench_disks(3)
    scene = tmp_path / "disks.txt"
    with open(scene, "w") as f:
        for p, m in zip(g.points, g.normals):
            f.write(" ".join(float(v).hex() for v in list(p) + list(m)) + "\n")
    flags = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include",
             "-I", os.path.join(ROOT, "include", "viennaray_amd"), "-I", os.path.join(ROOT, "include")]
    src = os.path.join(ROOT, "tests", "aux", "facade_radiosity.cpp")
    exe = tmp_path / "facade_radiosity"
    lib = os.path.join(ROOT, "viennaray_amd")
    subprocess.check_call(["g++", "-O1"] + flags + [src, "-o", str(exe), "-L", lib, "-lviennaray_amd",
                                                    "-L", "/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib,
                                                    "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe), str(scene)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "facade radiosity ok" in out.stdout, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    head = lines.index([l for l in lines if l.startswith("flux ")][0])
    _, its, rbits = lines[head].split()
    got = np.array([int(l, 16) for l in lines[head + 1:head + 1 + len(g.points)]], dtype=np.uint32)
    t = vr.TraceDisk(3)
    t.setGeometry(g.points, g.normals, 1.0)
    t.setBoundaryConditions(MESH_BCS)
    _prepared(t)
    want, w_its, w_res = t.solveRadiosity(256, sticking=0.25, returnInfo=True)
    assert (got == _bits(want)).all() and int(its) == w_its and int(rbits, 16) == int(_bits(np.float32(w_res))[0])
