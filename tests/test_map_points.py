"""Per-primitive values at the caller's points on the device (vr_map_to_points_device, vr_map_to_points,
vr_get_flux_at_points_device; Trace.mapToPoints / getFluxAtPoints) against the brute-force float64 reference of
tests/map_points_ref.py, on disks and triangles in two and three dimensions.

The bound of the weighted means, |out - ref| <= (K + 8) * 2^-23 * max|values| / min(1, sum_w), is derived from the float32
rounding of the K weights and of the two sums of non-negative terms; it is not measured.  Queries the reference calls
ambiguous (a centre within 1e-5 R of the radius, a sum of weights below 0.05, for nearest-only checks two nearest centres
within 1e-4 of each other) are left out of value comparisons, and every test that leaves any out asserts that they are
at most 2 % of its queries."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import viennaray_amd as vr
from viennaray_amd import capi
from helpers import DATA, trench2d, trench3d, trench_mesh

import map_points_ref as mp

pytestmark = pytest.mark.gpu

REF = vr.BoundaryCondition.REFLECTIVE_BOUNDARY
SOURCE = vr.NormalizationType.SOURCE
GEOMETRIES = ("disks3d", "disks2d", "mesh3d", "strips2d", "sheet300")
M = 1061  # not a multiple of 64
NEVER = "4294967295"


def _torch():
    import torch
    return torch


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def grid_mesh(nt, width=16, ripple=0.3, gd=1.0):
    """the first nt triangles of a grid of `width` cells per row, two triangles per cell, the vertices rippled by `ripple`
    grid cells"""
    cells = (nt + 1) // 2
    rows = (cells + width - 1) // width
    i, j = np.meshgrid(np.arange(rows + 1), np.arange(width + 1), indexing="ij")
    z = ripple * gd * np.sin(0.9 * j) * np.cos(0.7 * i)
    v = np.stack([j.ravel() * gd, i.ravel() * gd, z.ravel()], axis=1).astype(np.float32)
    c = np.arange(cells)
    a = (c // width) * (width + 1) + c % width
    b, d, e = a + 1, a + width + 1, a + width + 2
    t = np.empty((2 * cells, 3), dtype=np.uint32)
    t[0::2] = np.stack([a, b, d], 1)
    t[1::2] = np.stack([b, e, d], 1)
    return gd, v, np.ascontiguousarray(t[:nt])


def geometry(name):
    """dict(kind, D, gd, and the arrays setGeometry takes)"""
    if name == "disks3d":
        gd, p, n = trench3d()
        return dict(kind="disk", D=3, gd=gd, points=p, normals=n)
    if name == "disks2d":
        gd, p, n = trench2d()
        return dict(kind="disk", D=2, gd=gd, points=p, normals=n)
    if name == "mesh3d":
        gd, v, t = trench_mesh()
        return dict(kind="tri", D=3, gd=gd, verts=v, tris=t)
    if name == "strips2d":
        gd, nodes, lines = vr.io.read_line_mesh(os.path.join(DATA, "lineMesh.dat"))
        v, t, _ = vr.io.lines_to_triangles(nodes, lines, gd)
        return dict(kind="tri", D=2, gd=gd, verts=v, tris=t)
    gd, v, t = grid_mesh(300, ripple=0.1)  # (gentler than the default: the normals of a neighbourhood within 5 degrees)
    return dict(kind="tri", D=3, gd=gd, verts=v, tris=t)


def centres_of(g):
    """the primitive centres as the library takes them, float32 [n, 3]"""
    if g["kind"] == "disk":
        return np.ascontiguousarray(g["points"], dtype=np.float32).reshape(-1, 3)
    return mp.triangle_centroids(g["verts"], g["tris"])


def new_tracer(g, rays=4000, sticking=1.0, apply=True, collect=True):
    t = vr.TraceDisk(g["D"]) if g["kind"] == "disk" else vr.TraceTriangle(g["D"])
    if g["kind"] == "disk":
        t.setGeometry(g["points"], g["normals"], g["gd"])
    else:
        t.setGeometry(g["verts"], g["tris"], g["gd"])
    t.setBoundaryConditions([REF] * g["D"])
    t.setParticleType(vr.DiffuseParticle(sticking, "flux"))
    t.setNumberOfRaysFixed(rays)
    t.setUseRandomSeeds(False)
    t.setRngSeed(4711)
    if apply:
        t.apply(collect=collect)
    return t


@functools.lru_cache(maxsize=None)
def scene(name):
    """one tracer per geometry with one apply() behind it (a scene build is resident), and what the reference needs"""
    g = geometry(name)
    t = new_tracer(g)
    c = centres_of(g)
    nrm = np.asarray(g["normals"], dtype=np.float32) if g["kind"] == "disk" else t.debugTriangleMesh()[0]
    return dict(g=g, t=t, D=g["D"], gd=g["gd"], centres=c, normals=nrm, n=c.shape[0])


def _tilted(rng, nrm, D):
    """unit vectors tilted away from the rows of nrm by a random angle of up to 100 degrees (in the plane for D == 2):
    85 % of them by 0 .. 65 degrees, the others by 97 .. 100 degrees, past the horizon.  (The band around 90 degrees, where
    every gate is nearly shut, is what the reference calls ambiguous: drawn uniformly, one query in twenty has a sum of
    weights below 0.05 at R = gridDelta, which alone would break the 2 % cap.)"""
    n = np.asarray(nrm, dtype=np.float64).copy()
    if D == 2:
        n[:, 2] = 0.0
    n /= np.linalg.norm(n, axis=1)[:, None]
    if D == 2:
        t = np.stack([-n[:, 1], n[:, 0], np.zeros(len(n))], 1) * rng.choice([-1.0, 1.0], len(n))[:, None]
    else:
        r = rng.normal(size=n.shape)
        t = r - (r * n).sum(1)[:, None] * n
        t /= np.linalg.norm(t, axis=1)[:, None]
    deg = np.where(rng.uniform(size=len(n)) < 0.85, rng.uniform(0.0, 65.0, len(n)), rng.uniform(97.0, 100.0, len(n)))
    ang = np.deg2rad(deg)[:, None]
    return (n * np.cos(ang) + t * np.sin(ang)).astype(np.float32)


def _far_points(rng, centres, D, count=64, candidates=2048):
    """`count` points 64 scene sizes outside the box.  From that far the nearest centre is the one that reaches furthest
    along the viewing direction, and its lead over the runner-up, relative to the distance, is what separates the two
    smallest squared distances: of `candidates` random directions the `count` with the largest lead are kept, so that the
    reference can name the nearest centre (a random direction leaves nine of ten such queries ambiguous)."""
    c = centres.astype(np.float64)[:, :D]
    lo, hi = c.min(0), c.max(0)
    size = float(np.linalg.norm(hi - lo))
    u = rng.normal(size=(candidates, D))
    u /= np.linalg.norm(u, axis=1)[:, None]
    lead = np.empty(candidates)
    for k in range(0, candidates, 64):
        top = np.partition(c @ u[k:k + 64].T, c.shape[0] - 2, axis=0)[-2:]
        lead[k:k + 64] = top[1] - top[0]
    best = u[np.argsort(lead)[-count:]]
    far = np.zeros((count, 3))
    far[:, :D] = 0.5 * (lo + hi) + best * 64.0 * size
    if D == 2:
        far[:, 2] = centres[0, 2]
    return far.astype(np.float32)


@functools.lru_cache(maxsize=None)
def queries(name):
    """M centres jittered by +-0.4 gridDelta per axis, in random order, with their tilted normals and random values;
    `far`: 64 points 64 scene sizes outside the box"""
    s = scene(name)
    rng = np.random.default_rng(20240 + GEOMETRIES.index(name))
    own = rng.integers(0, s["n"], M)
    pts = (s["centres"][own].astype(np.float64) + rng.uniform(-0.4, 0.4, (M, 3)) * s["gd"]).astype(np.float32)
    nrm = _tilted(rng, s["normals"][own], s["D"])
    far = _far_points(rng, s["centres"], s["D"])
    values = rng.uniform(0.0, 1.0, s["n"]).astype(np.float32)
    return dict(points=pts, normals=nrm, far=far, far_normals=_tilted(rng, np.tile([[0.0, 1.0, 0.0]], (64, 1)), s["D"]),
                values=values)


@functools.lru_cache(maxsize=None)
def reference(name, radius_in_gd, gated, with_far=True):
    s, q = scene(name), queries(name)
    pts = np.concatenate([q["points"], q["far"]]) if with_far else q["points"]
    nrm = (np.concatenate([q["normals"], q["far_normals"]]) if with_far else q["normals"]) if gated else None
    return pts, nrm, mp.reference(q["values"], s["centres"], s["normals"], pts, nrm, radius_in_gd * s["gd"], D=s["D"])


def run(s, values, pts, nrm, radius):
    out = s["t"].mapToPoints(_dev(values), _dev(pts), None if nrm is None else _dev(nrm), radius)
    return out.cpu().numpy()


def assert_few(mask, what):
    share = float(np.mean(mask))
    print(f"{what}: {int(mask.sum())} of {mask.size} queries ambiguous ({100 * share:.2f} %)")
    assert share <= mp.MAX_AMBIGUOUS, (what, share)


def assert_identity(s):
    ids = np.arange(s["n"], dtype=np.float32)
    out = run(s, ids, s["centres"], None, 0.0)
    assert np.array_equal(out, ids), np.nonzero(out != ids)[0][:10]


# ---- 1. identity -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GEOMETRIES)
def test_identity_at_the_own_centres(name):
    """values[j] = j, the queries the primitives' own centres, R = 0: out[i] == i exactly"""
    assert_identity(scene(name))


# ---- 2. nearest ids --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GEOMETRIES)
def test_nearest_ids(name):
    s = scene(name)
    pts, _, ref = reference(name, 0.0, False)
    ids = np.arange(s["n"], dtype=np.float32)
    out = run(s, ids, pts, None, 0.0)
    keep = ~ref["ambiguous_nearest"]
    assert_few(~keep, f"nearest ids, {name}")
    assert np.array_equal(out[keep], ref["jstar"][keep].astype(np.float32)), np.nonzero(out[keep] != ref["jstar"][keep])[0][:10]
    k = int(np.nonzero(keep)[0][0])
    one = run(s, ids, pts[k:k + 1], None, 0.0)  # m = 1
    assert one.shape == (1,) and one[0] == float(ref["jstar"][k])


# ---- 3. weighted means -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gated", (False, True), ids=("plain", "normals"))
@pytest.mark.parametrize("radius", (1.0, 2.5))
@pytest.mark.parametrize("name", GEOMETRIES)
def test_weighted_means(name, radius, gated):
    s, q = scene(name), queries(name)
    pts, nrm, ref = reference(name, radius, gated)
    out = run(s, q["values"], pts, nrm, radius * s["gd"]).astype(np.float64)
    mean = ref["sum_w"] > 0
    # where the mean applies: the bound; where it does not (K == 0, every normal gated away): values[j*] exactly
    keep = np.where(mean, ~ref["ambiguous"], ~ref["ambiguous_nearest"])
    assert_few(~keep, f"weighted means, {name}, R = {radius} gridDelta, {'normals' if gated else 'plain'}")
    err = np.abs(out - ref["out"])
    tol = mp.tolerance(ref, q["values"])
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = float(np.max(np.where(keep & mean, err / tol, 0.0)))
    print(f"  largest |out - ref| {float(err[keep & mean].max(initial=0.0)):.3e}, {worst:.3f} of its bound; "
          f"K up to {int(ref['K'].max())}, fallbacks {int((keep & ~mean).sum())}")
    assert (err[keep] <= tol[keep]).all(), (int((err[keep] > tol[keep]).sum()), worst)
    exact = keep & ~mean
    assert np.array_equal(out[exact], q["values"][ref["jstar"][exact]].astype(np.float64))


# ---- 4. everything in range ------------------------------------------------------------------------------------------
def test_everything_in_range():
    s, q = scene("sheet300"), queries("sheet300")
    R = 10.0 * float(np.linalg.norm(s["centres"].max(0) - s["centres"].min(0)))
    ref = mp.reference(q["values"], s["centres"], s["normals"], q["points"], None, R, D=3)
    assert (ref["K"] == s["n"]).all() and s["n"] == 300
    out = run(s, q["values"], q["points"], None, R).astype(np.float64)
    keep = ~ref["ambiguous"]
    assert_few(~keep, "everything in range")
    err, tol = np.abs(out - ref["out"]), mp.tolerance(ref, q["values"])
    print(f"  largest |out - ref| {float(err[keep].max()):.3e}, {float((err / tol)[keep].max()):.3f} of its bound")
    assert (err[keep] <= tol[keep]).all()


# ---- 5. D == 2 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("disks2d", "strips2d"))
def test_two_dimensions_ignore_z(name):
    s, q = scene(name), queries(name)
    rng = np.random.default_rng(5)
    p0, n0 = q["points"].copy(), q["normals"].copy()
    p0[:, 2] = 0.0
    n0[:, 2] = 0.0
    pz, nz = p0.copy(), n0.copy()
    pz[:, 2] = rng.normal(size=M) * 1e3
    nz[:, 2] = rng.normal(size=M) * 1e3
    for R in (0.0, 2.5 * s["gd"]):
        for gated in (False, True):
            a = run(s, q["values"], p0, n0 if gated else None, R)
            b = run(s, q["values"], pz, nz if gated else None, R)
            c = run(s, q["values"], p0[:, :2], n0[:, :2] if gated else None, R)  # ld == 2
            assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(c)), (R, gated)


# ---- 6. sort path ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("disks3d", "mesh3d"))
def test_sorted_and_unsorted_queries_give_the_same_bits(name, monkeypatch):
    """the accumulation of a query follows its walk, not the launch order; m = 70 001 takes the sort's multi-block path"""
    s, q = scene(name), queries(name)
    rng = np.random.default_rng(6)
    lo, hi = s["centres"].min(0), s["centres"].max(0)
    big = (lo + (hi - lo) * rng.uniform(-0.05, 1.05, (70_001, 3))).astype(np.float32)
    for pts in (np.concatenate([q["points"], q["far"]])[:M], big):
        nrm = _tilted(rng, np.tile([[0.0, 0.0, 1.0]], (len(pts), 1)), 3)
        for R, gate in ((0.0, None), (2.5 * s["gd"], None), (2.5 * s["gd"], nrm)):
            monkeypatch.setenv("VR_MAP_SORT_MIN", "0")
            a = run(s, q["values"], pts, gate, R)
            monkeypatch.setenv("VR_MAP_SORT_MIN", NEVER)
            b = run(s, q["values"], pts, gate, R)
            assert np.array_equal(_bits(a), _bits(b)), (len(pts), R, gate is not None)
            assert not np.isnan(a).any()


# ---- 7. non-finite queries -------------------------------------------------------------------------------------------
def test_rows_that_are_not_finite_give_nan_and_leave_the_others_alone(monkeypatch):
    s, q = scene("disks3d"), queries("disks3d")
    pts = q["points"][:208].copy()
    want = run(s, q["values"], pts, None, 2.5 * s["gd"])
    rows = np.array([3, 40, 64, 65, 127, 128, 190, 207])
    bad = pts.copy()
    for k, (r, v) in enumerate(zip(rows, (np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf, np.nan, np.inf))):
        bad[r, k % 3] = v
    for sort in ("0", NEVER):
        monkeypatch.setenv("VR_MAP_SORT_MIN", sort)
        got = run(s, q["values"], bad, None, 2.5 * s["gd"])  # (returns: VR_OK)
        assert np.isnan(got[rows]).all()
        ok = np.setdiff1d(np.arange(208), rows)
        assert np.array_equal(_bits(got[ok]), _bits(want[ok]))
    assert_identity(s)


# ---- 8. flux path ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ks", (("disks3d", (0, 1)), ("mesh3d", (0,))))
def test_flux_at_the_own_centres_is_the_flux(name, ks):
    g = geometry(name)
    c = _dev(centres_of(g))
    for collect in (True, False):
        t = new_tracer(g, rays=20_000, sticking=0.1, collect=collect)
        for k in ks:
            want = t.getFluxTensor(0, SOURCE, k)
            got = t.getFluxAtPoints(c, radius=0.0, norm=SOURCE, numNeighbors=k)
            assert got.is_cuda and np.array_equal(_bits(got.cpu().numpy()), _bits(want.cpu().numpy())), (collect, k)
            assert float(want.abs().sum()) > 0
    host = t.getFluxAtPoints(centres_of(g), radius=0.0, norm=SOURCE)  # numpy in, numpy out
    assert isinstance(host, np.ndarray) and np.array_equal(_bits(host), _bits(t.getFluxTensor(0, SOURCE, 0).cpu().numpy()))


def test_host_form_equals_device_form():
    s, q = scene("mesh3d"), queries("mesh3d")
    pts, nrm = np.concatenate([q["points"], q["far"]]), np.concatenate([q["normals"], q["far_normals"]])
    for gate in (None, nrm):
        dev = run(s, q["values"], pts, gate, 2.5 * s["gd"])
        host = s["t"].mapToPoints(q["values"], pts, gate, 2.5 * s["gd"])
        assert isinstance(host, np.ndarray) and np.array_equal(_bits(host), _bits(dev))
    # radius=None means 2 * gridDelta
    assert np.array_equal(_bits(s["t"].mapToPoints(q["values"], pts)), _bits(run(s, q["values"], pts, None, 2.0 * s["gd"])))
    assert s["t"].mapToPoints(q["values"], np.empty((0, 3), np.float32)).shape == (0,)  # m == 0


# ---- 9. refusals -----------------------------------------------------------------------------------------------------
def _call(t, values, n, pts, nrm, m, ld, radius, out):
    ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data)
    rc = t._L.vr_map_to_points_device(t._h, ptr(values), n, ptr(pts), ptr(nrm), m, ld, radius, ptr(out), None)
    return rc, t._L.vr_last_error(t._h).decode()


def test_refusals_leave_out_untouched_and_the_context_usable():
    torch = _torch()
    g = geometry("disks3d")
    c = centres_of(g)
    n = c.shape[0]
    vals, pts = _dev(np.arange(n, dtype=np.float32)), _dev(c)
    out = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")

    def refused(t, code, word, *args):
        rc, msg = _call(t, *args)
        torch.cuda.synchronize()
        assert rc == code and word in msg, (rc, msg)
        assert bool((out == -7.0).all())

    t = new_tracer(g, apply=False)
    refused(t, capi.VR_E_STATE, "no scene build", vals, n, pts, None, n, 3, 0.0, out)  # before any apply
    with pytest.raises(vr.VrError):
        t.getFluxAtPoints(pts, radius=0.0)
    t.apply()
    refused(t, capi.VR_E_INVALID, "size mismatch", vals, n - 1, pts, None, n, 3, 0.0, out)
    refused(t, capi.VR_E_INVALID, "ld is 2 or 3", vals, n, pts, None, n, 4, 0.0, out)
    refused(t, capi.VR_E_INVALID, "2-D scene", vals, n, pts, None, n, 2, 0.0, out)
    refused(t, capi.VR_E_INVALID, "radius", vals, n, pts, None, n, 3, -1.0, out)
    refused(t, capi.VR_E_INVALID, "radius", vals, n, pts, None, n, 3, float("nan"), out)
    refused(t, capi.VR_E_INVALID, "device memory", vals, n, c, None, n, 3, 0.0, out)  # a host pointer as points
    refused(t, capi.VR_E_INVALID, "null", vals, n, None, None, n, 3, 0.0, out)
    rc, _ = _call(t, vals, n, pts, None, 0, 3, 0.0, out)  # m == 0: fine, nothing touched
    assert rc == capi.VR_OK and bool((out == -7.0).all())
    rc, _ = _call(t, vals, n, pts, None, n, 3, 0.0, out)  # and a valid call gives the identity
    torch.cuda.synchronize()
    assert rc == capi.VR_OK and torch.equal(out, vals)
    # the geometry set anew, no apply since: the resident build is the previous geometry's
    out.fill_(-7.0)
    t.setGeometry(g["points"], g["normals"], g["gd"])
    refused(t, capi.VR_E_STATE, "no scene build", vals, n, pts, None, n, 3, 0.0, out)
    t.apply()
    rc, _ = _call(t, vals, n, pts, None, n, 3, 0.0, out)
    torch.cuda.synchronize()
    assert rc == capi.VR_OK and torch.equal(out, vals)
    # tensors that cannot go as they are
    for bad in (pts.double(), pts.cpu(), pts.t().contiguous().t()):
        with pytest.raises(ValueError):
            t.mapToPoints(vals, bad, None, 0.0)
        with pytest.raises(ValueError):
            t.getFluxAtPoints(bad, radius=0.0)
    with pytest.raises(ValueError):
        t.mapToPoints(vals.double(), pts, None, 0.0)
    with pytest.raises(ValueError):
        t.mapToPoints(vals, pts, pts.double(), 0.0)
    assert torch.equal(t.mapToPoints(vals, pts, None, 0.0), vals)
