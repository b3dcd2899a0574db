"""gatherPaths on the device (vr_gather_paths, vr_gather_paths_device, vr_debug_gather_path; Trace.gatherPaths,
Trace.debugGatherPath): gatherFlux's samples followed back through their reflections.  Identity with gatherFlux bit for
bit where nothing can bounce, same bits over range splits and entry points, single paths reproduced vertex by vertex
through castRays and numpy float32, the specular trench bottom against its mirror-image closed form and the diffuse
trench against the radiosity system per triangle (bounds derived: Bhatia-Davis for weights in [0, 1], the reference's own
error and the truncation at maxBounces), the power cosine on the FINAL direction, per-primitive reflectivities, the
refusals, and an apply left as it was.  The scenes are those of tests/closed_forms.py, built as tests/test_gather_flux.py
builds them."""
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
K = 4096
ONE = np.float32(1.0)
RHO = np.float32(0.7)
KINDS = [GR.SPECULAR, GR.DIFFUSE]


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
def _mesh():
    g = cf.trench_mesh()
    cen, _ = cf.triangle_centroids(g)
    coord = np.where(g.part == cf.BOTTOM, cen[:, 0], cen[:, 2])  # x on the bottom, z on the walls (unused on the top)
    return _prepared(_mesh_tracer(g)), g, coord


@functools.lru_cache(maxsize=None)
def _mesh_deep():
    """the trench mesh with a wall budget no path of the tests below can spend"""
    g = cf.trench_mesh()
    t = _mesh_tracer(g)
    t.setMaxBoundaryHits(1 << 16)
    return _prepared(t), g


@functools.lru_cache(maxsize=None)
def _disks2():
    g = cf.trench_disks(2)
    t = vr.TraceDisk(2)
    t.setGeometry(g.points, g.normals, 1.0)
    t.setBoundaryConditions([BC.REFLECTIVE_BOUNDARY, BC.REFLECTIVE_BOUNDARY])
    t.setSourceDirection(cf.POS_Y)
    return _prepared(t), g


@functools.lru_cache(maxsize=None)
def _flat(bc):
    n = 16
    i, j = np.meshgrid(np.arange(n, dtype=np.float32), np.arange(n, dtype=np.float32), indexing="ij")
    pts = np.stack([i.ravel(), j.ravel(), np.zeros(n * n, np.float32)], 1)
    nrm = np.tile(np.array([0, 0, 1], np.float32), (n * n, 1))
    t = vr.TraceDisk(3)
    t.setGeometry(pts, nrm, 1.0)
    t.setBoundaryConditions([bc, bc, bc])
    return _prepared(t)


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gather_paths") / "gather_paths")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I",
                           os.path.join(ROOT, "viennaray_amd", "csrc"), os.path.join(ROOT, "tests", "aux", "gather_paths.cpp"), "-o", exe])
    return exe


def _host_lines(exe, args, rows):
    text = "\n".join(" ".join(v if isinstance(v, str) else float(v).hex() for v in row) for row in rows)
    out = subprocess.run([exe] + args, input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return np.array([[float.fromhex(v) for v in line.split()] for line in out.stdout.splitlines()], dtype=np.float32)


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


def _result(weights, samples):
    """q(), the int64 sum and gather_result of vr_gather.hpp in numpy"""
    w = np.minimum(np.asarray(weights, dtype=np.float32), np.float32(2.0 ** 22 / samples))  # (samples: a power of two here)
    q = np.where(w > 0, (w.astype(np.float64) * 2.0 ** 40 + 0.5).astype(np.int64), 0)
    return np.float32(float(q.sum()) / 2.0 ** 40 / samples)


# ---------------------------------------------------------------------------------------------------------------
# 1. identity: where nothing can bounce the result is gatherFlux's, bit for bit
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["mesh", "disks2"])
@pytest.mark.parametrize("samples", [64, 100])
@pytest.mark.parametrize("power", [1.0, 8.0])
def test_no_bounce_is_gather_flux(scene, samples, power):
    t = _mesh()[0] if scene == "mesh" else _disks2()[0]
    want = t.gatherFlux(samples, cosinePower=power, numpy=True)
    assert (want > 0).any() and (want < 1).any()
    for kind in KINDS:
        a = t.gatherPaths(samples, reflectivity=0.7, reflection=kind, maxBounces=0, cosinePower=power, numpy=True)
        b = t.gatherPaths(samples, reflectivity=0.0, reflection=kind, maxBounces=8, cosinePower=power, numpy=True)
        assert (_bits(a) == _bits(want)).all() and (_bits(b) == _bits(want)).all(), (scene, samples, power, kind)


@pytest.mark.parametrize("bc", [BC.PERIODIC_BOUNDARY, BC.REFLECTIVE_BOUNDARY])
def test_flat_surface_is_exactly_one_for_any_bounce_budget(bc):
    for kind in KINDS:
        for bounces in (0, 1, 64):
            out = _flat(bc).gatherPaths(100, reflectivity=0.7, reflection=kind, maxBounces=bounces, numpy=True)
            assert out.shape == (256,) and (_bits(out) == _bits(ONE)).all()


# ---------------------------------------------------------------------------------------------------------------
# 2. same bits for splits and entry points
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_same_bits_over_ranges_and_entry_points(kind):
    import torch
    t, g, _ = _mesh()
    n = len(g.tris)
    kw = dict(reflectivity=0.7, reflection=kind, maxBounces=5)
    whole = t.gatherPaths(100, numpy=True, **kw)
    assert (whole > t.gatherFlux(100, numpy=True)).any()  # (something bounced)
    again = t.gatherPaths(100, numpy=True, **kw)
    assert (_bits(whole) == _bits(again)).all()
    parts = np.concatenate([t.gatherPaths(100, primFirst=a, primCount=b - a, numpy=True, **kw) for a, b in ((0, 3), (3, 73), (73, n))])
    assert (_bits(parts) == _bits(whole)).all()
    dev = t.gatherPaths(100, **kw)
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and (_bits(dev.cpu().numpy()) == _bits(whole)).all()
    table = t.gatherPaths(100, reflectivity=np.full(n, 0.7, np.float32), reflection=kind, maxBounces=5)
    assert isinstance(table, np.ndarray) and (_bits(table) == _bits(whole)).all()
    stick = t.gatherPaths(100, sticking=torch.full((n,), 0.3, device="cuda"), reflection=kind, maxBounces=5)
    assert isinstance(stick, torch.Tensor) and (_bits(stick.cpu().numpy()) == _bits(whole)).all()  # (1 - 0.3f == 0.7f)
    for prim in (0, 77, n - 1):  # a range of one primitive: its chunks are cut into sub-runs
        one = t.gatherPaths(100, primFirst=prim, primCount=1, numpy=True, **kw)
        assert one.shape == (1,) and _bits(one)[0] == _bits(whole)[prim], prim
    assert t.gatherPaths(100, primFirst=5, primCount=0, numpy=True, **kw).shape == (0,)


# ---------------------------------------------------------------------------------------------------------------
# 3. one path, reproduced
# ---------------------------------------------------------------------------------------------------------------
def _np_reflect(d, n):
    """reflect_specular of vr_math.hpp, float32, in its operation order"""
    inv = -d
    f = np.float32(2) * ((n[:, 0] * inv[:, 0] + n[:, 1] * inv[:, 1]) + n[:, 2] * inv[:, 2])
    return f[:, None] * n - inv


def _test_prims(g):
    return int(np.nonzero(g.part == cf.BOTTOM)[0][3]), int(np.nonzero(g.part == cf.LEFT)[0][11])


def _paths(t, prim, count, **kw):
    return [t.debugGatherPath(prim, k, **kw) for k in range(count)]


def _check_chain(t, prim, paths):
    """every leaving direction, cast from its vertex, lands on the next vertex; returns the number of segments checked"""
    org, dirs, want_id, want_pt = [], [], [], []
    for p in paths:
        v = len(p["ids"])
        assert v == p["numVertices"] and p["ids"][0] == prim and p["end"] != capi.VR_GATHER_END_WALL
        assert np.isnan(p["arriving"][0]).all() and not np.isnan(p["leaving"][:v - 1]).any()
        ended_on_vertex = bool(np.isnan(p["leaving"][v - 1]).any())
        assert ended_on_vertex == (p["end"] in (capi.VR_GATHER_END_BACK, capi.VR_GATHER_END_BOUNCES, capi.VR_GATHER_END_ABSORBED))
        # only PERIODIC walls are passed between two vertices of this scene: a direction arrives as it left
        assert (_bits(p["arriving"][1:]) == _bits(p["leaving"][:v - 1])).all()
        last = v - 1 if ended_on_vertex else v
        for k in range(last):
            org.append(p["points"][k])
            dirs.append(p["leaving"][k])
            want_id.append(int(p["ids"][k + 1]) if k + 1 < v else capi.VR_CAST_MISS)
            want_pt.append(p["points"][k + 1] if k + 1 < v else np.full(3, np.nan, np.float32))
        final = p["leaving"][v - 1] if not ended_on_vertex else p["arriving"][v - 1]
        # (above the trench a path may still meet a REFLECTIVE wall in x on its way to the source: that mirrors x alone)
        assert (_bits(np.abs(p["direction"])) == _bits(np.abs(final))).all() and (_bits(p["direction"][1:]) == _bits(final[1:])).all()
    hit, _, pts = t.castRays(np.array(org, np.float32), np.array(dirs, np.float32), returnPoints=True)
    want_id, want_pt = np.array(want_id), np.array(want_pt, np.float32)
    assert (hit == want_id).all(), np.nonzero(hit != want_id)[0][:10]
    geo = want_id >= 0
    assert (_bits(pts[geo]) == _bits(want_pt[geo])).all()
    return len(org)


def _np_weights(paths, rho_of, max_bounces):
    """T by float32 multiplies and the end -> weight rule at power 1 (g = 1), from the vertices alone"""
    ws = []
    for p in paths:
        v = len(p["ids"])
        T, bounces, end = ONE, 0, None
        for k in range(1, v):
            front = float((p["arriving"][k].astype(np.float32) * p["normals"][k]).astype(np.float32).sum(dtype=np.float64)) < 0
            if not front or bounces >= max_bounces:
                end = "vertex"
                break
            T = np.float32(T * rho_of(int(p["ids"][k])))
            if T == 0:
                end = "vertex"
                break
            bounces += 1
        assert (end == "vertex") == bool(np.isnan(p["leaving"][v - 1]).any())
        reached = end is None and p["end"] == capi.VR_GATHER_END_MISS and p["direction"][2] > 0  # u = +z
        w = T if reached else np.float32(0)
        assert _bits(T)[0] == _bits(p["throughput"])[0] and _bits(w)[0] == _bits(p["weight"])[0]
        ws.append(w)
    return np.array(ws, np.float32)


def test_specular_paths_reproduced_vertex_by_vertex():
    t, g = _mesh_deep()
    kw = dict(reflectivity=float(RHO), reflection=GR.SPECULAR, maxBounces=48)
    segments = 0
    for prim in _test_prims(g):
        paths = _paths(t, prim, 256, **kw)
        _, _, d0 = t.debugGatherSamples(prim, 0, 256)
        assert (_bits(np.array([p["leaving"][0] for p in paths])) == _bits(d0)).all()
        arr = np.concatenate([p["arriving"][1:][~np.isnan(p["leaving"][1:]).any(1)] for p in paths])
        nrm = np.concatenate([p["normals"][1:][~np.isnan(p["leaving"][1:]).any(1)] for p in paths])
        out = np.concatenate([p["leaving"][1:][~np.isnan(p["leaving"][1:]).any(1)] for p in paths])
        assert len(out) > 100 and (_bits(out) == _bits(_np_reflect(arr, nrm))).all()
        segments += _check_chain(t, prim, paths)
        assert max(p["numVertices"] for p in paths) >= 3  # (more than one bounce somewhere)
        w = _np_weights(paths, lambda j: RHO, 48)
        got = t.gatherPaths(256, primFirst=prim, primCount=1, numpy=True, **kw)
        assert _bits(got)[0] == _bits(_result(w, 256))[0], (prim, got)
    print("specular: %d segments reproduced through castRays" % segments)


def test_diffuse_paths_reproduced_and_drawn_as_the_host_program_draws(host_program):
    t, g = _mesh_deep()
    kw = dict(reflectivity=float(RHO), reflection=GR.DIFFUSE, maxBounces=48)
    for prim in _test_prims(g):
        paths = _paths(t, prim, 256, **kw)
        _, _, d0 = t.debugGatherSamples(prim, 0, 256)
        assert (_bits(np.array([p["leaving"][0] for p in paths])) == _bits(d0)).all()
        rows, out = [], []
        for k, p in enumerate(paths):
            for v in range(1, len(p["ids"])):
                if not np.isnan(p["leaving"][v]).any():  # bounce v - 1 of sample k
                    rows.append([str(prim), str(k), str(v - 1)] + list(p["normals"][v]))
                    out.append(p["leaving"][v])
        assert len(out) > 100
        assert (_bits(np.array(out)) == _bits(_host_lines(host_program, ["dirs", str(SEED), "3"], rows))).all()
        _check_chain(t, prim, paths)
        w = _np_weights(paths, lambda j: RHO, 48)
        got = t.gatherPaths(256, primFirst=prim, primCount=1, numpy=True, **kw)
        assert _bits(got)[0] == _bits(_result(w, 256))[0], (prim, got)


# ---------------------------------------------------------------------------------------------------------------
# 4., 5. closed forms per triangle
# ---------------------------------------------------------------------------------------------------------------
def test_specular_trench_bottom_per_triangle():
    """mirror images of the opening, image k through |k| reflections of weight 0.7: cf.specular_bottom at the centroid.
    Weights lie in [0, 1] (Bhatia-Davis); paths cut at B bounces lack at most 0.7^(B + 1)"""
    s, B = 0.3, 48
    t, g, coord = _mesh()
    out = t.gatherPaths(K, sticking=s, reflection=GR.SPECULAR, maxBounces=B, numpy=True)
    top, b = g.part == cf.TOP, g.part == cf.BOTTOM
    assert (_bits(out[top]) == _bits(ONE)).all()
    F = cf.specular_bottom(cf.W, cf.DEPTH, s, coord[b])
    _check("specular bottom s=0.3", out[b], F, _bd(F, 1.0) + 0.7 ** (B + 1))


def test_diffuse_trench_per_triangle():
    """the radiosity system of the trench at sticking 0.2, interpolated to the centroids as test_radiosity_fixed_point
    does"""
    s, B = 0.2, 64
    t, g, coord = _mesh()
    out = t.gatherPaths(K, sticking=s, reflection=GR.DIFFUSE, maxBounces=B, numpy=True)
    R = cf.radiosity(s=s)
    F = np.ones(len(g.tris))
    for p in (cf.BOTTOM, cf.LEFT, cf.RIGHT):
        sel, seg = g.part == p, R.part == p
        mid = 0.5 * (R.lo[seg] + R.hi[seg])
        order = np.argsort(mid)
        F[sel] = np.interp(coord[sel], mid[order], R.F[seg][order])
    top = g.part == cf.TOP
    assert (_bits(out[top]) == _bits(ONE)).all()
    _check("diffuse s=0.2", out[~top], F[~top], _bd(F[~top], 1.0) + cf.REFERENCE_ERROR + 0.8 ** (B + 1))


# ---------------------------------------------------------------------------------------------------------------
# 6. the power cosine is taken of the FINAL direction
# ---------------------------------------------------------------------------------------------------------------
def test_power_cosine_weighs_the_final_direction(host_program):
    t, g = _mesh_deep()
    n = 8.0
    changed = 0
    for prim in _test_prims(g):
        paths = _paths(t, prim, 256, reflectivity=1.0, reflection=GR.SPECULAR, maxBounces=1, cosinePower=n)
        rows_end = [[str(p["end"]), p["direction"][2], p["throughput"]] for p in paths]  # u = +z
        rows_first = [[str(p["end"]), p["leaving"][0][2], p["throughput"]] for p in paths]
        w_end = _host_lines(host_program, ["weights", "3", float(n).hex()], rows_end)[:, 0]
        w_first = _host_lines(host_program, ["weights", "3", float(n).hex()], rows_first)[:, 0]
        got = np.array([p["weight"] for p in paths], np.float32)
        assert (_bits(got) == _bits(w_end)).all()
        changed += int((_bits(w_end) != _bits(w_first)).sum())
        assert all(p["throughput"] == 1 for p in paths)
        res = t.gatherPaths(256, reflectivity=1.0, reflection=GR.SPECULAR, maxBounces=1, cosinePower=n, primFirst=prim, primCount=1,
                            numpy=True)
        assert _bits(res)[0] == _bits(_result(got, 256))[0]
    assert changed > 20, changed  # (paths that reached the source after a bounce: their c is not the initial one)


# ---------------------------------------------------------------------------------------------------------------
# 7. per-primitive reflectivity
# ---------------------------------------------------------------------------------------------------------------
def test_per_primitive_reflectivity():
    import torch
    t, g = _mesh_deep()
    n = len(g.tris)
    rho = np.where(g.part == cf.LEFT, RHO, np.float32(0)).astype(np.float32)
    kw = dict(reflection=GR.SPECULAR, maxBounces=48)
    host = t.gatherPaths(256, reflectivity=rho, **kw)
    dev = t.gatherPaths(256, reflectivity=torch.from_numpy(rho).cuda(), **kw)
    assert isinstance(host, np.ndarray) and isinstance(dev, torch.Tensor) and dev.is_cuda
    assert (_bits(dev.cpu().numpy()) == _bits(host)).all()
    stick = t.gatherPaths(256, sticking=(ONE - rho).astype(np.float32), **kw)
    assert (_bits(stick) == _bits(host)).all()
    direct = t.gatherFlux(256, numpy=True)
    assert (host >= direct).all() and (host > direct).any()
    right = g.part == cf.RIGHT  # the right wall faces the only mirror
    assert (host[right] > direct[right]).any()
    for prim in (int(np.nonzero(g.part == cf.BOTTOM)[0][3]), int(np.nonzero(right)[0][11])):
        paths = _paths(t, prim, 256, reflectivity=rho, **kw)
        w = _np_weights(paths, lambda j: rho[j], 48)
        assert _bits(host)[prim] == _bits(_result(w, 256))[0], prim


# ---------------------------------------------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------------------------------------------
def _raw(t, first, count, samples, power, reflection, bounces, table, scalar, out):
    fp = C.POINTER(C.c_float)
    return t._L.vr_gather_paths(t._h, first, count, samples, power, reflection, bounces,
                                table.ctypes.data_as(fp) if table is not None else None, scalar,
                                out.ctypes.data_as(fp) if out is not None else None)


def test_refusals_leave_out_untouched_and_the_context_usable():
    import torch
    t, g, _ = _mesh()
    n = len(g.tris)
    poison = np.float32(-123.5)
    want = t.gatherPaths(64, reflectivity=0.7, maxBounces=5, numpy=True)
    nan, inf = float("nan"), float("inf")
    bad_low = np.full(n, 0.5, np.float32)
    bad_low[[17, 300]] = [-0.25, 2.0]
    bad_nan = np.full(n, 0.5, np.float32)
    bad_nan[41] = np.nan
    cases = [  # first, count, samples, power, reflection, bounces, table, scalar
        (0, n, 0, 1.0, 0, 5, None, 0.7), (1, n, 64, 1.0, 0, 5, None, 0.7), (n, 1, 64, 1.0, 0, 5, None, 0.7),
        (0, n, 64, 0.5, 0, 5, None, 0.7), (0, n, 64, nan, 0, 5, None, 0.7), (0, n, 64, inf, 0, 5, None, 0.7),
        (0, n, (1 << 22) + 1, 1.0, 0, 5, None, 0.7), (0, n, 1 << 20, 8.0, 0, 5, None, 0.7),
        (0, n, 64, 1.0, 2, 5, None, 0.7), (0, n, 64, 1.0, 0, 65536, None, 0.7),
        (0, n, 64, 1.0, 0, 5, None, nan), (0, n, 64, 1.0, 0, 5, None, -0.125), (0, n, 64, 1.0, 1, 5, None, 1.5),
        (0, n, 64, 1.0, 0, 5, bad_low, 0.7), (0, n, 64, 1.0, 1, 5, bad_nan, 0.7)]
    for case in cases:
        out = np.full(n, poison, np.float32)
        assert _raw(t, *case, out) == capi.VR_E_INVALID, case[:6]
        assert (out == poison).all() and t._L.vr_last_error(t._h)
    # a bad table entry is named by its lowest index
    out = np.full(n, poison, np.float32)
    assert _raw(t, 0, n, 64, 1.0, 0, 5, bad_low, 0.7, out) == capi.VR_E_INVALID
    assert b"reflectivity[17]" in t._L.vr_last_error(t._h)
    with pytest.raises(vr.VrError, match=r"reflectivity\[41\]"):
        t.gatherPaths(64, reflectivity=torch.from_numpy(bad_nan).cuda())
    with pytest.raises(vr.VrError, match=r"reflectivity\[17\]"):
        t.debugGatherPath(0, 0, reflectivity=bad_low)
    for prim, sample in ((n, 0), (0, 1 << 22)):  # a primitive beyond the scene, a sample beyond any call's
        with pytest.raises(vr.VrError):
            t.debugGatherPath(prim, sample, reflectivity=0.7)
    last = t.debugGatherPath(n - 1, (1 << 22) - 1, reflectivity=0.7, maxBounces=3)  # (the last sample there can be)
    assert last["numVertices"] >= 1 and last["ids"][0] == n - 1
    assert _raw(t, 0, n, 64, 1.0, 0, 5, None, 0.7, None) == capi.VR_E_INVALID  # out null
    assert _raw(t, 0, 0, 64, 1.0, 0, 5, None, 0.7, None) == capi.VR_OK  # nothing to do, after the checks
    assert _raw(t, 0, n, 64, 1.0, 0, 65535, None, 1.0, np.empty(n, np.float32)) == capi.VR_OK  # the limits themselves
    # the device form refuses host memory, for out and for the table
    host = np.full(n, poison, np.float32)
    dev = torch.full((n,), float(poison), device="cuda")
    L = t._L
    good = np.full(n, 0.5, np.float32)
    assert L.vr_gather_paths_device(t._h, 0, n, 64, 1.0, 0, 5, None, 0.7, C.c_void_p(host.ctypes.data), None) == capi.VR_E_INVALID
    assert L.vr_gather_paths_device(t._h, 0, n, 64, 1.0, 0, 5, C.c_void_p(good.ctypes.data), 0.0, C.c_void_p(dev.data_ptr()),
                                    None) == capi.VR_E_INVALID
    bad_dev = torch.from_numpy(bad_low).cuda()
    assert L.vr_gather_paths_device(t._h, 0, n, 64, 1.0, 0, 5, C.c_void_p(bad_dev.data_ptr()), 0.0, C.c_void_p(dev.data_ptr()),
                                    None) == capi.VR_E_INVALID
    torch.cuda.synchronize()
    assert (host == poison).all() and bool((dev == float(poison)).all())
    with pytest.raises(ValueError):
        t.gatherPaths(64)
    with pytest.raises(ValueError):
        t.gatherPaths(64, sticking=0.3, reflectivity=0.7)
    with pytest.raises(ValueError):
        t.gatherPaths(64, reflectivity=torch.zeros(n, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        t.gatherPaths(64, reflectivity=np.zeros(n - 1, np.float32))
    # ... and the context still answers
    assert (_bits(t.gatherPaths(64, reflectivity=0.7, maxBounces=5, numpy=True)) == _bits(want)).all()


def test_a_path_gather_needs_what_a_prepare_left_for_the_settings_in_force():
    g = cf.trench_mesh()
    n = len(g.tris)
    want = _mesh()[0].gatherPaths(64, reflectivity=0.7, maxBounces=5, numpy=True)
    t = _mesh_tracer(g)
    t.setParticleType(vr.DiffuseParticle(1.0, "flux"))
    t.setNumberOfRaysFixed(1000)
    t.setRngSeed(SEED)
    poison = np.float32(-123.5)

    def refused():
        import torch
        out = np.full(n, poison, np.float32)
        assert _raw(t, 0, n, 64, 1.0, 0, 5, None, 0.7, out) == capi.VR_E_STATE and (out == poison).all()
        dev = torch.full((n,), float(poison), device="cuda")
        assert t._L.vr_gather_paths_device(t._h, 0, n, 64, 1.0, 1, 5, None, 0.7, C.c_void_p(dev.data_ptr()), None) == capi.VR_E_STATE
        torch.cuda.synchronize()
        assert bool((dev == float(poison)).all())
        with pytest.raises(vr.VrError, match="nothing to gather from"):
            t.gatherPaths(64, reflectivity=0.7, numpy=True)
        with pytest.raises(vr.VrError, match="nothing to gather from"):
            t.debugGatherPath(0, 0, reflectivity=0.7)

    refused()  # before any prepare
    t.applyPrepare()
    assert (_bits(t.gatherPaths(64, reflectivity=0.7, maxBounces=5, numpy=True)) == _bits(want)).all()
    t.setBoundaryConditions([BC.PERIODIC_BOUNDARY, BC.IGNORE_BOUNDARY, BC.REFLECTIVE_BOUNDARY])  # other walls
    refused()
    t.setBoundaryConditions([BC.REFLECTIVE_BOUNDARY, BC.PERIODIC_BOUNDARY, BC.REFLECTIVE_BOUNDARY])
    t.applyPrepare()
    assert (_bits(t.gatherPaths(64, reflectivity=0.7, maxBounces=5, numpy=True)) == _bits(want)).all()


def test_the_wall_budget_counts_over_the_whole_path():
    """a budget of one wall: a path may pass one wall in all, not one per segment"""
    g = cf.trench_mesh()
    t = _mesh_tracer(g)
    t.setMaxBoundaryHits(1)
    _prepared(t)
    prim = _test_prims(g)[1]
    paths = _paths(t, prim, 256, reflectivity=1.0, reflection=GR.SPECULAR, maxBounces=48)
    deep, _ = _mesh_deep()
    free = _paths(deep, prim, 256, reflectivity=1.0, reflection=GR.SPECULAR, maxBounces=48)
    stopped = [k for k, p in enumerate(paths) if p["end"] == capi.VR_GATHER_END_WALL]
    assert len(stopped) > 0 and all(p["weight"] == 0 for p in (paths[k] for k in stopped))
    later = 0
    for k in stopped:  # the same path without a budget goes further; with it, it had passed exactly one wall before
        assert free[k]["numVertices"] >= paths[k]["numVertices"]
        later += int(paths[k]["numVertices"] > 1)
    assert later > 0  # (stopped behind a reflection: the count was not reset there)
    for k in set(range(256)) - set(stopped):
        assert paths[k]["numVertices"] == free[k]["numVertices"] and _bits(paths[k]["weight"])[0] == _bits(free[k]["weight"])[0]


# ---------------------------------------------------------------------------------------------------------------
# 9. an apply is untouched
# ---------------------------------------------------------------------------------------------------------------
def _apply_twice(paths_between):
    g = cf.trench_mesh()
    t = _mesh_tracer(g)
    t.setParticleType(vr.DiffuseParticle(0.3, "flux"))
    t.setNumberOfRaysFixed(200_000)
    t.setRngSeed(SEED)
    t.setUseRandomSeeds(False)
    t.apply()
    first = np.array(t.getLocalData().getVectorData("flux"))
    if paths_between:
        t.gatherPaths(128, reflectivity=0.7, numpy=True)
        t.gatherPaths(64, sticking=np.full(len(g.tris), 0.2, np.float32), reflection=GR.DIFFUSE, cosinePower=8.0)
        t.debugGatherPath(5, 3, reflectivity=0.7)
        assert (_bits(t.getLocalData().getVectorData("flux")) == _bits(first)).all()
    t.apply()
    return first, np.array(t.getLocalData().getVectorData("flux")), t.getRayTraceInfo().as_dict()


def test_an_apply_is_untouched_by_a_path_gather():
    f0, s0, i0 = _apply_twice(False)
    f1, s1, i1 = _apply_twice(True)
    assert (_bits(f0) == _bits(f1)).all() and (_bits(s0) == _bits(s1)).all()
    skip = {"time", "timeBuild", "timeTrace", "timeTraceKernel", "timeGenKernel"}
    assert {k: v for k, v in i0.items() if k not in skip} == {k: v for k, v in i1.items() if k not in skip}


# ---------------------------------------------------------------------------------------------------------------
# 10. the C++ façade
# ---------------------------------------------------------------------------------------------------------------
def test_cpp_facade_gather_paths(tmp_path):
    """tests/aux/facade_gather_paths.cpp on a sheet of disks folded into V grooves; the values it prints are the Python
    call's on the same scene, bit for bit"""
    flags = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include",
             "-I", os.path.join(ROOT, "include", "viennaray_amd"), "-I", os.path.join(ROOT, "include")]
    src = os.path.join(ROOT, "tests", "aux", "facade_gather_paths.cpp")
    exe = tmp_path / "facade_gather_paths"
    lib = os.path.join(ROOT, "viennaray_amd")
    subprocess.check_call(["g++", "-O1"] + flags + [src, "-o", str(exe), "-L", lib, "-lviennaray_amd",
                                                    "-L", "/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib,
                                                    "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "facade gather paths ok" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    printed = {line.split()[0]: np.array([float.fromhex(v) for v in line.split()[1:]], np.float32)
               for line in out.stdout.splitlines() if line.startswith(("specular", "diffuse"))}
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
    for name, kind in (("specular", GR.SPECULAR), ("diffuse", GR.DIFFUSE)):
        got = t.gatherPaths(64, sticking=0.3, reflection=kind, maxBounces=8, numpy=True)
        assert printed[name].shape == got.shape and (_bits(printed[name]) == _bits(got)).all(), name
