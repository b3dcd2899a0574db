"""gatherFlux on the device (vr_gather_flux, vr_gather_flux_device, vr_debug_gather_samples; Trace.gatherFlux): rays cast
FROM every primitive into its hemisphere, against point-exact closed forms of tests/closed_forms.py — no oracle run, no
recorded scatter.  Exact values (an unoccluded flat surface is 1.0f bit for bit), same bits over calls, range splits and
entry points, the direct flux of the trench per primitive within 5 sigma of a Bhatia-Davis variance bound, the power
cosine source in both sampling modes, one radiosity iteration at its fixed point, the sample directions against the host
program bit for bit, and the refusals."""
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
GM = vr.GatherMode
SEED = 7
K = 4096
ONE = np.float32(1.0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _prepared(t):
    t.setParticleType(vr.DiffuseParticle(1.0, "flux"))
    t.setNumberOfRaysFixed(1000)
    t.setRngSeed(SEED)
    t.applyPrepare()
    return t


@functools.lru_cache(maxsize=None)
def _mesh():
    g = cf.trench_mesh()
    t = vr.TraceTriangle(3)
    t.setGeometry(g.verts, g.tris, 1.0)
    t.setBoundaryConditions([BC.REFLECTIVE_BOUNDARY, BC.PERIODIC_BOUNDARY, BC.REFLECTIVE_BOUNDARY])
    cen, _ = cf.triangle_centroids(g)
    coord = np.where(g.part == cf.BOTTOM, cen[:, 0], cen[:, 2])  # x on the bottom, z on the walls (unused on the top)
    return _prepared(t), g, coord


@functools.lru_cache(maxsize=None)
def _disks2():
    g = cf.trench_disks(2)
    t = vr.TraceDisk(2)
    t.setGeometry(g.points, g.normals, 1.0)
    t.setBoundaryConditions([BC.REFLECTIVE_BOUNDARY, BC.REFLECTIVE_BOUNDARY])
    t.setSourceDirection(cf.POS_Y)
    return _prepared(t), g


@functools.lru_cache(maxsize=None)
def _flat(bc, flipped=False):
    n = 16
    i, j = np.meshgrid(np.arange(n, dtype=np.float32), np.arange(n, dtype=np.float32), indexing="ij")
    pts = np.stack([i.ravel(), j.ravel(), np.zeros(n * n, np.float32)], 1)
    nrm = np.tile(np.array([0, 0, 1], np.float32), (n * n, 1))
    t = vr.TraceDisk(3)
    t.setGeometry(pts, nrm, 1.0)
    t.setBoundaryConditions([bc, bc, bc])
    if flipped:
        t.setSourceDirection(vr.TraceDirection.NEG_Z)
    return _prepared(t)


@functools.lru_cache(maxsize=None)
def _mesh_normal_1():
    """the one K = 4096, n = 1 gather of the trench mesh several tests look at"""
    t, _, _ = _mesh()
    return t.gatherFlux(K, numpy=True)


def _check(name, got, ref, bound):
    got, ref, bound = (np.asarray(a, dtype=np.float64) for a in (got, ref, bound))
    err = np.abs(got - ref)
    k = int(np.argmax(err / bound))
    print("%s: %d primitives, worst uses %.0f %% of its bound (got %.5f ref %.5f bound %.5f)"
          % (name, len(got), 100 * err[k] / bound[k], got[k], ref[k], bound[k]))
    bad = np.nonzero(~(err <= bound))[0]
    assert len(bad) == 0, [(int(q), float(got[q]), float(ref[q]), float(bound[q])) for q in bad[:10]]


def _bd(F, g, k=K):
    """5 sigma of a mean of k samples in [0, g] with expectation F (Bhatia-Davis: var <= F (g - F))"""
    F = np.asarray(F, dtype=np.float64)
    return 5.0 * np.sqrt(np.clip(F * (g - F), 0.0, None) / k) + 1e-5


# ---------------------------------------------------------------------------------------------------------------
# 1. exact values
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bc", [BC.PERIODIC_BOUNDARY, BC.REFLECTIVE_BOUNDARY])
@pytest.mark.parametrize("samples", [64, 100])
def test_flat_surface_is_exactly_one(bc, samples):
    out = _flat(bc).gatherFlux(samples, numpy=True)
    assert out.shape == (256,) and out.dtype == np.float32
    assert (_bits(out) == _bits(ONE)).all(), out[out != 1][:8]


def test_flat_surface_facing_away_is_zero():
    out = _flat(BC.PERIODIC_BOUNDARY, True).gatherFlux(64, numpy=True)
    assert (_bits(out) == 0).all()


def test_ignore_walls_lose_samples():
    """through an IGNORE wall a sample leaves for good: strictly between 0 and 1 somewhere, never above 1"""
    out = _flat(BC.IGNORE_BOUNDARY).gatherFlux(256, numpy=True)
    assert (out <= 1).all() and (out < 1).any() and (out > 0).all()


def test_emission_of_zeros_is_no_emission():
    t, g, _ = _mesh()
    out = t.gatherFlux(K, emission=np.zeros(len(g.tris), np.float32))
    assert (_bits(out) == _bits(_mesh_normal_1())).all()


# ---------------------------------------------------------------------------------------------------------------
# 2. same bits
# ---------------------------------------------------------------------------------------------------------------
def test_same_bits_over_calls_ranges_and_entry_points():
    import torch
    t, g, _ = _mesh()
    n = len(g.tris)
    a, b = t.gatherFlux(128, numpy=True), t.gatherFlux(128, numpy=True)
    assert (_bits(a) == _bits(b)).all()
    third = n // 3
    parts = np.concatenate([t.gatherFlux(128, primFirst=0, primCount=third, numpy=True),
                            t.gatherFlux(128, primFirst=third, numpy=True)])
    assert (_bits(parts) == _bits(a)).all()
    dev = t.gatherFlux(128)
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and (_bits(dev.cpu().numpy()) == _bits(a)).all()
    # an emission table: numpy in, numpy out; tensor in, tensor out
    em = np.linspace(0.0, 0.5, n).astype(np.float32)
    h = t.gatherFlux(128, emission=em)
    d = t.gatherFlux(128, emission=torch.from_numpy(em).cuda())
    assert isinstance(h, np.ndarray) and isinstance(d, torch.Tensor) and (_bits(d.cpu().numpy()) == _bits(h)).all()
    assert (h >= a).all() and (h > a).any()
    one = t.gatherFlux(128, primFirst=n - 1, primCount=1, numpy=True)
    assert one.shape == (1,) and _bits(one)[0] == _bits(a)[-1]
    assert t.gatherFlux(128, primFirst=5, primCount=0, numpy=True).shape == (0,)


def _apply_twice(gather_between):
    g = cf.trench_mesh()
    t = vr.TraceTriangle(3)
    t.setGeometry(g.verts, g.tris, 1.0)
    t.setBoundaryConditions([BC.REFLECTIVE_BOUNDARY, BC.PERIODIC_BOUNDARY, BC.REFLECTIVE_BOUNDARY])
    t.setParticleType(vr.DiffuseParticle(0.3, "flux"))
    t.setNumberOfRaysFixed(200_000)
    t.setRngSeed(SEED)
    t.setUseRandomSeeds(False)
    t.apply()
    first = np.array(t.getLocalData().getVectorData("flux"))
    if gather_between:
        t.gatherFlux(128, numpy=True)
        t.gatherFlux(64, cosinePower=8.0, mode=GM.SOURCE)
        assert (_bits(t.getLocalData().getVectorData("flux")) == _bits(first)).all()
    t.apply()
    return first, np.array(t.getLocalData().getVectorData("flux")), t.getRayTraceInfo().as_dict()


def test_an_apply_is_untouched_by_a_gather():
    f0, s0, i0 = _apply_twice(False)
    f1, s1, i1 = _apply_twice(True)
    assert (_bits(f0) == _bits(f1)).all() and (_bits(s0) == _bits(s1)).all()
    skip = {"time", "timeBuild", "timeTrace", "timeTraceKernel", "timeGenKernel"}
    assert {k: v for k, v in i0.items() if k not in skip} == {k: v for k, v in i1.items() if k not in skip}


# ---------------------------------------------------------------------------------------------------------------
# 3. closed forms, NORMAL, n = 1, per primitive
# ---------------------------------------------------------------------------------------------------------------
def test_trench_mesh_direct_flux_per_triangle():
    _, g, coord = _mesh()
    out = _mesh_normal_1()
    top = g.part == cf.TOP
    assert (_bits(out[top]) == _bits(ONE)).all()
    F = cf.radiosity().direct_at(g.part[~top], coord[~top])[0]
    _check("mesh direct", out[~top], F, _bd(F, 1.0))


def test_trench_disks_2d_direct_flux_per_disk():
    t, g = _disks2()
    out = t.gatherFlux(K, numpy=True)
    keep = g.part != cf.TOP
    for p, c in cf.disk_excluded(g):
        keep &= ~((g.part == p) & (g.coord == c))
    assert keep.sum() >= 24
    F = cf.radiosity().direct_at(g.part[keep], g.coord[keep])[0]
    _check("disks2 direct", out[keep], F, _bd(F, 1.0))


# ---------------------------------------------------------------------------------------------------------------
# 4. power cosine
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,n", [(GM.NORMAL, 8.0), (GM.SOURCE, 8.0), (GM.SOURCE, 50.0)])
def test_power_cosine_bottom(mode, n):
    t, g, coord = _mesh()
    out = t.gatherFlux(K, cosinePower=n, mode=mode, numpy=True)
    b = g.part == cf.BOTTOM
    F = cf.power_cosine_bottom(cf.W, cf.DEPTH, n, coord[b])
    # NORMAL: w in [0, g], g = (n + 1) / 2; SOURCE on the bottom: m = u, so w is 0 or 1
    _check("power %g %s" % (n, mode.name), out[b], F, _bd(F, (n + 1) / 2 if mode == GM.NORMAL else 1.0))


def _wall_source_flux(n, z, steps):
    """Flux at depth z < 0 of a side wall under the cos^n source, float64 midpoint rule in the polar angle theta from u:
    (n + 1) / (2 pi) int cos^(n-1) sin^2 I(theta) dtheta, I the integral of cos(phi) over the azimuths whose ray leaves
    through the opening of width W: tan(theta) cos(phi) < W / |z| (y is periodic: no bound there) — 2, or
    2 (1 - sqrt(1 - a^2)) where a = W / (|z| tan(theta)) < 1"""
    th = (np.arange(steps) + 0.5) * (np.pi / 2 / steps)
    a = cf.W / (np.abs(z)[:, None] * np.tan(th)[None, :])
    inner = np.where(a >= 1.0, 2.0, 2.0 * (1.0 - np.sqrt(np.clip(1.0 - a * a, 0.0, None))))
    f = np.cos(th)[None, :] ** (n - 1) * np.sin(th)[None, :] ** 2 * inner
    return (n + 1) / (2 * np.pi) * f.sum(1) * (np.pi / 2 / steps)


def test_power_cosine_walls_source_mode():
    n = 8.0
    t, g, coord = _mesh()
    out = t.gatherFlux(K, cosinePower=n, mode=GM.SOURCE, numpy=True)
    wall = (g.part == cf.LEFT) | (g.part == cf.RIGHT)
    F, F2 = _wall_source_flux(n, coord[wall], 4000), _wall_source_flux(n, coord[wall], 8000)
    assert np.abs(F - F2).max() < 5e-4, np.abs(F - F2).max()  # (the 2e-3 below covers the quadrature)
    # n = 1 against the closed form: the quadrature itself
    F1 = _wall_source_flux(1.0, coord[wall], 8000)
    assert np.abs(F1 - cf.radiosity().direct_at(g.part[wall], coord[wall])[0]).max() < 5e-4
    _check("power 8 SOURCE walls", out[wall], F2, np.full(F2.shape, 5.0 * np.sqrt(1.0 / (n - 1) / K) + 2e-3))


# ---------------------------------------------------------------------------------------------------------------
# 5. the radiosity fixed point
# ---------------------------------------------------------------------------------------------------------------
def test_radiosity_fixed_point():
    """emission = (1 - s) F of the solved system at every centroid (R's convention: F is the INCOMING flux; the flat top
    re-emits nothing that comes back, emission 0 there): one gather returns F"""
    s = 0.2
    t, g, coord = _mesh()
    R = cf.radiosity(s=s)
    F = np.ones(len(g.tris))
    for p in (cf.BOTTOM, cf.LEFT, cf.RIGHT):
        sel, seg = g.part == p, R.part == p
        mid = 0.5 * (R.lo[seg] + R.hi[seg])
        order = np.argsort(mid)
        F[sel] = np.interp(coord[sel], mid[order], R.F[seg][order])
    em = np.where(g.part == cf.TOP, 0.0, (1 - s) * F).astype(np.float32)
    out = t.gatherFlux(K, emission=em)
    top = g.part == cf.TOP
    assert (_bits(out[top]) == _bits(ONE)).all()
    M = max(1.0, float(em.max()))
    _check("radiosity s=0.2", out[~top], F[~top], _bd(F[~top], M) + cf.REFERENCE_ERROR)


# ---------------------------------------------------------------------------------------------------------------
# 6. directions
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gather") / "gather")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I",
                           os.path.join(ROOT, "viennaray_amd", "csrc"), os.path.join(ROOT, "tests", "aux", "gather.cpp"), "-o", exe])
    return exe


def _host_dirs(exe, prim, chunk, m, mode, n):
    # the mesh tracer's frame: source towards +z, plane axes x and y
    args = [str(SEED), str(prim), str(chunk)] + [float(v).hex() for v in m] + [str(int(mode)), "3", repr(float(n)), "2", "0", "1", "1"]
    out = subprocess.run([exe, "dirs"] + args, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    return np.array([[float.fromhex(v) for v in line.split()] for line in out.stdout.splitlines()], dtype=np.float32)


@pytest.mark.parametrize("mode,n", [(GM.NORMAL, 1.0), (GM.SOURCE, 8.0)])
def test_directions_match_the_host_program_and_a_cast_reproduces_the_gather(mode, n, host_program):
    t, g, _ = _mesh()
    cen, _ = cf.triangle_centroids(g)
    for prim in (int(np.nonzero(g.part == cf.BOTTOM)[0][3]), int(np.nonzero(g.part == cf.LEFT)[0][11])):
        o, m, d = t.debugGatherSamples(prim, 0, 256, mode, n)
        assert np.abs(o - cen[prim]).max() < 1e-5 and abs(float(np.linalg.norm(m)) - 1) < 1e-6
        for chunk in (0, 3):
            assert (_bits(d[64 * chunk:64 * chunk + 64]) == _bits(_host_dirs(host_program, prim, chunk, m, mode, n))).all(), (prim, chunk)
        o2, m2, d2 = t.debugGatherSamples(prim, 192, 64, mode, n)
        assert (_bits(d2) == _bits(d[192:])).all() and (_bits(o2) == _bits(o)).all() and (_bits(m2) == _bits(m)).all()
        # the same rays through castRays, the weight rule in numpy, the int64 quantisation
        hit, _ = t.castRays(np.tile(o, (256, 1)), d, followBoundaries=True)
        c = d[:, 2]  # u = +z
        if mode == GM.NORMAL:
            w = np.where((hit == capi.VR_CAST_MISS) & (c > 0), ONE, np.float32(0))
        else:
            mw = ((m[0] * d[:, 0] + m[1] * d[:, 1]).astype(np.float32) + m[2] * d[:, 2]).astype(np.float32)
            walked = mw > 0
            with np.errstate(divide="ignore", invalid="ignore"):
                w = np.where(walked & (hit == capi.VR_CAST_MISS) & (c > 0), (mw / c).astype(np.float32), np.float32(0))
        w = np.minimum(w, np.float32(2.0 ** 22 / 256))  # (wmax of 256 samples: a weight above it counts wmax)
        q = np.where(w > 0, (w.astype(np.float64) * 2.0 ** 40 + 0.5).astype(np.int64), 0)
        ref = np.float32(float(q.sum()) / 2.0 ** 40 / 256)
        got = t.gatherFlux(256, cosinePower=n, mode=mode, primFirst=prim, primCount=1, numpy=True)
        assert _bits(got)[0] == _bits(ref)[0], (prim, got, ref)


# ---------------------------------------------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------------------------------------------
def _raw(t, first, count, samples, power, mode, emission, out):
    fp = C.POINTER(C.c_float)
    return t._L.vr_gather_flux(t._h, first, count, samples, power, mode,
                               emission.ctypes.data_as(fp) if emission is not None else None,
                               out.ctypes.data_as(fp) if out is not None else None)


def test_refusals_leave_out_untouched_and_the_context_usable():
    import torch
    t, g, _ = _mesh()
    n = len(g.tris)
    em = np.zeros(n, np.float32)
    poison = np.float32(-123.5)
    cases = [(0, n, 0, 1.0, 0, None), (1, n, 64, 1.0, 0, None), (n, 1, 64, 1.0, 0, None), (0, n, 64, 0.5, 0, None),
             (0, n, 64, float("nan"), 0, None), (0, n, 64, float("inf"), 0, None), (0, n, 64, 1.0, 2, None),
             (0, n, 64, 1.5, 1, None), (0, n, 64, 8.0, 1, em)]
    for first, count, samples, power, mode, e in cases:
        out = np.full(n, poison, np.float32)
        assert _raw(t, first, count, samples, power, mode, e, out) == capi.VR_E_INVALID, (first, count, samples, power, mode)
        assert (out == poison).all() and t._L.vr_last_error(t._h)
    assert _raw(t, 0, n, 64, 1.0, 0, None, None) == capi.VR_E_INVALID
    assert _raw(t, 0, 0, 64, 1.0, 0, None, None) == capi.VR_OK  # nothing to do, after the checks
    # the device form refuses host memory
    host = np.full(n, poison, np.float32)
    dev = torch.full((n,), float(poison), device="cuda")
    L = t._L
    assert L.vr_gather_flux_device(t._h, 0, n, 64, 1.0, 0, None, C.c_void_p(host.ctypes.data), None) == capi.VR_E_INVALID
    assert L.vr_gather_flux_device(t._h, 0, n, 64, 1.0, 0, C.c_void_p(em.ctypes.data), C.c_void_p(dev.data_ptr()), None) == capi.VR_E_INVALID
    torch.cuda.synchronize()
    assert (host == poison).all() and bool((dev == float(poison)).all())
    with pytest.raises(ValueError):
        t.gatherFlux(64, emission=torch.zeros(n, dtype=torch.float64, device="cuda"))
    # nothing prepared: VR_E_STATE
    fresh = vr.TraceTriangle(3)
    fresh.setGeometry(g.verts, g.tris, 1.0)
    out = np.full(n, poison, np.float32)
    assert _raw(fresh, 0, n, 64, 1.0, 0, None, out) == capi.VR_E_STATE and (out == poison).all()
    o3, d3 = np.zeros(3, np.float32), np.zeros((4, 3), np.float32)
    fp = C.POINTER(C.c_float)
    assert fresh._L.vr_debug_gather_samples(fresh._h, 0, 0, 4, 0, 1.0, o3.ctypes.data_as(fp), o3.ctypes.data_as(fp),
                                            d3.ctypes.data_as(fp)) == capi.VR_E_STATE
    # ... and the context still answers
    assert (_bits(t.gatherFlux(K, numpy=True)) == _bits(_mesh_normal_1())).all()


def _state_tracer(g):
    t = vr.TraceTriangle(3)
    t.setGeometry(g.verts, g.tris, 1.0)
    t.setBoundaryConditions([BC.REFLECTIVE_BOUNDARY, BC.PERIODIC_BOUNDARY, BC.REFLECTIVE_BOUNDARY])
    t.setParticleType(vr.DiffuseParticle(1.0, "flux"))
    t.setNumberOfRaysFixed(1000)
    t.setRngSeed(SEED)
    return t


def _assert_state_refused(t, count):
    """every entry point answers VR_E_STATE and leaves a poisoned out as it is; count: a range valid for the geometry set"""
    import torch
    poison = np.float32(-123.5)
    with pytest.raises(vr.VrError, match="nothing to gather from"):
        t.gatherFlux(64, numpy=True)
    with pytest.raises(vr.VrError, match="nothing to gather from"):
        t.gatherFlux(64)
    out = np.full(count, poison, np.float32)
    assert _raw(t, 0, count, 64, 1.0, 0, None, out) == capi.VR_E_STATE and (out == poison).all()
    assert _raw(t, 0, count, 64, 8.0, 1, None, out) == capi.VR_E_STATE and (out == poison).all()
    dev = torch.full((count,), float(poison), device="cuda")
    assert t._L.vr_gather_flux_device(t._h, 0, count, 64, 1.0, 0, None, C.c_void_p(dev.data_ptr()), None) == capi.VR_E_STATE
    torch.cuda.synchronize()
    assert bool((dev == float(poison)).all())
    fp = C.POINTER(C.c_float)
    o3, m3, d3 = (np.full(s, poison, np.float32) for s in (3, 3, (4, 3)))
    assert t._L.vr_debug_gather_samples(t._h, 0, 0, 4, 0, 1.0, o3.ctypes.data_as(fp), m3.ctypes.data_as(fp),
                                        d3.ctypes.data_as(fp)) == capi.VR_E_STATE
    assert (o3 == poison).all() and (m3 == poison).all() and (d3 == poison).all()


def test_a_gather_needs_what_a_prepare_left_for_the_settings_in_force(monkeypatch):
    g = cf.trench_mesh()
    n = len(g.tris)
    want = _mesh()[0].gatherFlux(64, numpy=True)
    t = _state_tracer(g)

    def works():
        assert (_bits(t.gatherFlux(64, numpy=True)) == _bits(want)).all()

    _assert_state_refused(t, n)  # before any prepare
    t.apply()
    works()
    t.setGeometry(g.verts, g.tris[:-2], 1.0)  # another geometry
    _assert_state_refused(t, n - 2)
    t.setGeometry(g.verts, g.tris, 1.0)
    _assert_state_refused(t, n)  # (set anew: the resident build is the previous geometry's)
    t.apply()
    works()
    t.setBoundaryConditions([BC.PERIODIC_BOUNDARY, BC.IGNORE_BOUNDARY, BC.REFLECTIVE_BOUNDARY])  # other walls
    _assert_state_refused(t, n)
    t.setBoundaryConditions([BC.REFLECTIVE_BOUNDARY, BC.PERIODIC_BOUNDARY, BC.REFLECTIVE_BOUNDARY])
    t.apply()
    works()
    t.setSourceDirection(vr.TraceDirection.NEG_Z)  # u, the walls and the child order follow it
    _assert_state_refused(t, n)
    t.setSourceDirection(vr.TraceDirection.POS_Z)
    t.applyPrepare()  # a prepare is enough
    works()
    # a scene of the host builder has no pair nodes to walk: refused, though an apply has finished
    monkeypatch.setenv("VR_HOST_BUILD", "1")
    h = _state_tracer(g)
    h.apply()
    assert float(np.sum(h.getLocalData().getVectorData("flux"))) > 0
    _assert_state_refused(h, n)
    monkeypatch.delenv("VR_HOST_BUILD")
    h.setGeometry(g.verts, g.tris, 1.0)  # (the next scene build is the device's)
    _assert_state_refused(h, n)
    h.apply()
    assert (_bits(h.gatherFlux(64, numpy=True)) == _bits(want)).all()


def test_weights_above_wmax_are_cut_and_sums_cannot_overflow():
    """an emission table of huge values: every front-side hit counts wmax = 2^22 / 4096 = 1024, nothing wraps"""
    t, g, _ = _mesh()
    n = len(g.tris)
    base = _mesh_normal_1()
    hits = t.gatherFlux(K, emission=np.ones(n, np.float32)) - base          # the share of samples landing on a front
    for big in (1024.0, 3e38, float("inf")):
        out = t.gatherFlux(K, emission=np.full(n, big, np.float32))
        assert np.isfinite(out).all() and (out >= base).all()
        assert np.abs(out - (base + 1024.0 * hits)).max() <= 1e-3 * 1024.0, big
    # a NORMAL weight may not be cut: samples x g below 2^22
    out = np.full(n, -123.5, np.float32)
    assert _raw(t, 0, n, (1 << 22) + 1, 1.0, 0, None, out) == capi.VR_E_INVALID and (out == -123.5).all()
    assert _raw(t, 0, n, 1 << 20, 8.0, 0, None, out) == capi.VR_E_INVALID and (out == -123.5).all()


def test_cpp_facade_gather_flux(tmp_path):
    """tests/aux/facade_gather_flux.cpp: exact ones on a sheet of disks, the device form over two ranges word for word
    the host form, refusals"""
    flags = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include",
             "-I", os.path.join(ROOT, "include", "viennaray_amd"), "-I", os.path.join(ROOT, "include")]
    src = os.path.join(ROOT, "tests", "aux", "facade_gather_flux.cpp")
    exe = tmp_path / "facade_gather_flux"
    lib = os.path.join(ROOT, "viennaray_amd")
    subprocess.check_call(["g++", "-O1"] + flags + [src, "-o", str(exe), "-L", lib, "-lviennaray_amd",
                                                    "-L", "/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib,
                                                    "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "facade gather flux ok" in out.stdout, out.stdout + out.stderr
