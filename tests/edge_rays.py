"""Edge-case ray families and the scenes they are aimed at (plain module, no fixtures).

The tracer's exact primitive tests sit behind conservative culls (padded and quantised boxes, disc_may_hit, the
packet query's scene-box clip and wall pre-test, the relief clip); a cull that is too tight loses a hit without any
other symptom.  The families below put rays ON the margins of those culls: along the axes with signed zeros, grazing
the surface, on the rim of a disk, through mesh vertices and shared edges, at the line where a side wall meets the
surface, from far away, and again from the hit points themselves.  tests/test_edge_rays_oracle.py checks the oracle's
BVH walk against its own brute force on them, tests/test_edge_rays.py the device against that brute force.
"""
import collections
import functools

import numpy as np

import viennaray_amd as vr
from oracle import pyoracle as po
from helpers import trench2d, trench3d, trench_mesh

N = 1500  # rays per family

# lo / hi: the geometry's bounding box; centres: one point per primitive (disk centres, triangle centroids);
# radius: the disks' radius (meshes: gridDelta, the `r` of the rim family); verts / tris: meshes only.
# oracle: a prepared Oracle of the scene (its bbox() places the side walls, its brute force feeds `restart`).
Scene = collections.namedtuple("Scene", "name lo hi centres radius D up_axis verts tris normals gridDelta oracle")

SOURCE_SIDE = ("axis", "graze", "rim", "tiny", "wall_edge", "vertex_edge")  # usable as host rays
DEBUG_ONLY = ("restart", "far")                                            # origins inside / far outside the scene
SCENES = ("plane", "trench3d", "mesh", "trench2d", "coincident")
FLAT_SCENES = ("plane", "coincident")  # every primitive in one plane
RIM_EPS = (-1e-3, -1e-6, 0.0, 1e-6, 1e-3)
TINY = (1e-20, -1e-20, 1e-38, -1e-38, 1e-44, 1e-31, -1e-29, 0.0, 1e-3)
WALL_SHIFT = (0.0, 1e-6, -1e-6, 1e-3, -1e-3)

# trace modes each scene is expected to reach, by sticking (1.0: absorbing kernels, 0.3: general kernels)
MODES = {"plane": {1.0: 1, 0.3: 3}, "coincident": {1.0: 1, 0.3: 3}, "trench3d": {1.0: 2, 0.3: 0},
         "mesh": {1.0: 2, 0.3: 0}, "trench2d": {1.0: 4, 0.3: 4}}


def max_boundary_hits(family):
    """set explicitly on both sides: `graze` crosses hundreds of periodic walls before it lands; the in-plane rays of
    `axis` bounce between the side walls until this limit stops them"""
    return 50 if family == "axis" else 1000


def family_names(scene_name):
    return tuple(f for f in SOURCE_SIDE + DEBUG_ONLY if f != "vertex_edge" or scene_name == "mesh")


def source_side_names(scene_name):
    return tuple(f for f in SOURCE_SIDE if f != "vertex_edge" or scene_name == "mesh")


# ---------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------
def coincident_plane(n=40, gd=0.5):
    """A plane of disks in which every 7th disk appears three times: itself, an exact copy and a copy with the normal
    negated, both appended at the end: equal-t ties (the lower original id wins) and back faces."""
    pts, nrm = vr.io.plane_grid(n, gd)
    return (np.concatenate([pts, pts[::7], pts[::7]]).astype(np.float32),
            np.concatenate([nrm, nrm[::7], -nrm[::7]]).astype(np.float32))


@functools.lru_cache(maxsize=None)
def geometry(name):
    """(kind, D, gridDelta, a, b): disks -> a = points, b = normals; mesh -> a = vertices, b = triangles"""
    if name == "plane":
        p, n = vr.io.plane_grid(90, 0.5)
        return "disks", 3, 0.5, p, n
    if name == "coincident":
        p, n = coincident_plane()
        return "disks", 3, 0.5, p, n
    if name == "trench3d":
        gd, p, n = trench3d()
        return "disks", 3, gd, p, n
    if name == "trench2d":
        gd, p, n = trench2d()
        return "disks", 2, gd, p, n
    if name == "mesh":
        gd, v, tri = trench_mesh()
        return "mesh", 3, gd, v, tri
    raise KeyError(name)


def new_oracle(name, geom=None):
    kind, D, gd, a, b = geom if geom is not None else geometry(name)
    o = po.Oracle()
    if kind == "mesh":
        o.set_triangles(a, b, gd, D)
    else:
        o.set_disks(a, b, gd, D)
    if D == 2:
        o.set_source_direction(po.POS_Y)
    return o


def new_tracer(name, geom=None):
    kind, D, gd, a, b = geom if geom is not None else geometry(name)
    if kind == "mesh":
        t = vr.TraceTriangle(D)
    else:
        t = vr.TraceDisk(D)
    t.setGeometry(a, b, gd)
    if D == 2:
        t.setSourceDirection(vr.TraceDirection.POS_Y)
    return t


def boundary_conditions(D):
    BC = vr.BoundaryCondition
    if D == 2:
        return [BC.PERIODIC_BOUNDARY] * 2
    return [BC.REFLECTIVE_BOUNDARY, BC.PERIODIC_BOUNDARY, BC.REFLECTIVE_BOUNDARY]


@functools.lru_cache(maxsize=None)
def scene(name):
    kind, D, gd, a, b = geometry(name)
    o = new_oracle(name)
    o.prepare()
    up = 1 if D == 2 else 2
    if kind == "mesh":
        v = a.astype(np.float32)
        centres = ((v[b[:, 0]] + v[b[:, 1]] + v[b[:, 2]]) / np.float32(3)).astype(np.float32)
        return Scene(name, v.min(0), v.max(0), centres, np.float32(gd), D, up, v, b, o.normals(), gd, o)
    c = a.astype(np.float32).copy()
    nrm = b.astype(np.float32).copy()
    if D == 2:
        c[:, 2] = 0
        nrm[:, 2] = 0
    return Scene(name, c.min(0), c.max(0), c, np.float32(o.disk_radius()), D, up, None, None, nrm, gd, o)


# ---------------------------------------------------------------------------------------------------------------
# the families
# ---------------------------------------------------------------------------------------------------------------
def _unit32(s, d):
    """normalised in float64 (in 2-D: within the x-y plane), then rounded to float32"""
    d = np.array(d, dtype=np.float64)
    if s.D == 2:
        d[:, 2] = 0
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def _plan_axes(s):
    return [k for k in range(s.D) if k != s.up_axis]


def _finish(s, o, d):
    o = np.ascontiguousarray(o, dtype=np.float32)
    d = np.ascontiguousarray(d, dtype=np.float32)
    if s.D == 2:
        o[:, 2] = 0
        d[:, 2] = 0
    assert o.shape == d.shape == (N, 3)
    return o, d


def _axis(s, rng):
    """+-1 on one axis, +0.0 / -0.0 on the others; the origin is a primitive centre moved 3 units back along the ray, so
    the other two coordinates sit exactly on centre (and box) coordinates"""
    c = s.centres[rng.integers(0, len(s.centres), N)]
    ax = rng.integers(0, s.D, N)
    sign = rng.choice([-1.0, 1.0], N)
    d = np.where(rng.integers(0, 2, (N, 3)) == 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    d[np.arange(N), ax] = sign
    o = c.copy()
    o[np.arange(N), ax] = (c[np.arange(N), ax] - np.float32(3) * sign.astype(np.float32)).astype(np.float32)
    return o, d


def _graze(s, rng):
    """0.01 above the top, nearly parallel to it: the up component is -10^U(-7,-2) of a Gaussian plan direction"""
    o = rng.uniform(s.lo, s.hi, (N, 3)).astype(np.float32)
    o[:, s.up_axis] = np.float32(s.hi[s.up_axis]) + np.float32(0.01)
    d = np.zeros((N, 3))
    for k in _plan_axes(s):
        d[:, k] = rng.normal(size=N)
    d[:, s.up_axis] = -10.0 ** rng.uniform(-7, -2, N)
    return o, _unit32(s, d)


def _plane_basis(n, D):
    """two unit vectors spanning the plane with normal n (float64); in 2-D the second one is zero"""
    n = np.asarray(n, dtype=np.float64)
    n = n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-30)
    if D == 2:
        u = np.stack([-n[:, 1], n[:, 0], np.zeros(len(n))], -1)
        return u, np.zeros_like(u)
    helper = np.where(np.abs(n[:, [0]]) < 0.9, np.array([[1.0, 0, 0]]), np.array([[0, 1.0, 0]]))
    u = np.cross(n, helper)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return u, np.cross(n, u)


def _aim(s, rng, target, aside=1.0, above=2.0):
    """origins `above` over the targets (never below the top) and up to +-aside aside in plan; directions at the targets"""
    target = np.asarray(target, dtype=np.float64)
    o = target.copy()
    for k in _plan_axes(s):
        o[:, k] += rng.uniform(-aside, aside, len(target))
    o[:, s.up_axis] = np.maximum(target[:, s.up_axis] + above, float(s.hi[s.up_axis]))
    o = o.astype(np.float32)
    return o, _unit32(s, target - o.astype(np.float64))


def _rim(s, rng):
    """aimed at points at r (1 + eps) from a disk centre in the disk's plane (meshes: r = gridDelta around vertices, in
    the plane of a triangle that holds the vertex)"""
    if s.verts is None:
        i = rng.integers(0, len(s.centres), N)
        c, n = s.centres[i].astype(np.float64), s.normals[i]
    else:
        tri = rng.integers(0, len(s.tris), N)
        c = s.verts[s.tris[tri, rng.integers(0, 3, N)]].astype(np.float64)
        n = s.normals[tri]
    u, v = _plane_basis(n, s.D)
    phi = rng.uniform(0, 2 * np.pi, N)
    if s.D == 2:
        phi = np.where(rng.integers(0, 2, N) == 1, 0.0, np.pi)
    eps = np.asarray(RIM_EPS)[rng.integers(0, len(RIM_EPS), N)]
    rr = (float(s.radius) * (1.0 + eps))[:, None]
    target = c + rr * (np.cos(phi)[:, None] * u + np.sin(phi)[:, None] * v)
    return _aim(s, rng, target)


def _tiny(s, rng):
    """straight down with side components below and above safe_inverse's 1e-30 clamp, denormals included; half the
    origins exactly over a primitive centre"""
    c = s.centres[rng.integers(0, len(s.centres), N)].astype(np.float32)
    o = rng.uniform(s.lo, s.hi, (N, 3)).astype(np.float32)
    over = rng.integers(0, 2, N) == 1
    o[over] = c[over]
    o[:, s.up_axis] = np.float32(s.hi[s.up_axis]) + np.float32(1)
    d = np.zeros((N, 3))
    for k in _plan_axes(s):
        d[:, k] = np.asarray(TINY)[rng.integers(0, len(TINY), N)]
    d[:, s.up_axis] = -1.0
    return o, _unit32(s, d)


def _wall_edge(s, rng):
    """aimed at the line where a side wall of the oracle's bounding box meets the surface's mean height, displaced
    across the wall by 0, +-1e-6, +-1e-3"""
    bb = s.oracle.bbox().astype(np.float64)
    plan = _plan_axes(s)
    target = rng.uniform(bb[0], bb[1], (N, 3))
    target[:, s.up_axis] = float(np.mean(s.centres[:, s.up_axis].astype(np.float64)))
    k = np.asarray(plan)[rng.integers(0, len(plan), N)]
    side = rng.integers(0, 2, N)
    shift = np.asarray(WALL_SHIFT)[rng.integers(0, len(WALL_SHIFT), N)]
    target[np.arange(N), k] = bb[side, k] + shift
    o = rng.uniform(bb[0], bb[1], (N, 3))
    o[:, s.up_axis] = float(s.hi[s.up_axis]) + 1.0
    o = o.astype(np.float32)
    return o, _unit32(s, target - o.astype(np.float64))


def _vertex_edge(s, rng):
    """exactly at float32 vertices and (a + b) * 0.5f edge midpoints, half from straight above and half obliquely: equal-t
    ties between the triangles that share the vertex or edge"""
    tri = rng.integers(0, len(s.tris), N)
    e = rng.integers(0, 3, N)
    a = s.verts[s.tris[tri, e]]
    b = s.verts[s.tris[tri, (e + 1) % 3]]
    mid = ((a + b) * np.float32(0.5)).astype(np.float32)
    target = np.where((rng.integers(0, 2, N) == 1)[:, None], a, mid).astype(np.float32)
    o, d = _aim(s, rng, target, aside=1.0, above=1.0)
    above = np.arange(N) % 2 == 0
    o[above] = target[above]
    o[above, s.up_axis] = np.float32(s.hi[s.up_axis]) + np.float32(1)
    d[above] = 0
    d[above, s.up_axis] = -1
    return o, d


def brute_force(s, o, d):
    """the oracle's brute-force closest hit: (geomID i32, primID u32, t f32); misses have geomID -1"""
    return _intersect(s.oracle, o, d, True)


def _intersect(oracle, o, d, brute):
    n = len(o)
    g = np.full(n, -1, dtype=np.int32)
    p = np.zeros(n, dtype=np.uint32)
    t = np.zeros(n, dtype=np.float32)
    for i in range(n):
        h = oracle.intersect1(o[i], d[i], brute=brute)
        g[i] = h["geomID"]
        if h["geomID"] >= 0:
            p[i] = h["primID"]
            t[i] = h["t"]
    return g, p, t


def _restart(s, rng, fams):
    """from the float32 hit points o + d t of the oracle's geometry hits of `graze` and `rim`: in a random direction,
    exactly in the hit primitive's plane (cross(n, e_k), renormalised) and along the mirrored incoming direction"""
    o0 = np.concatenate([fams["graze"][0], fams["rim"][0]])
    d0 = np.concatenate([fams["graze"][1], fams["rim"][1]])
    g, p, t = brute_force(s, o0, d0)
    hit = np.flatnonzero(g == 1)
    assert len(hit) >= N // 10, (s.name, len(hit))
    i = hit[rng.integers(0, len(hit), N)]
    o = (o0[i] + d0[i] * t[i, None]).astype(np.float32)
    n = s.normals[p[i]].astype(np.float64)
    din = d0[i].astype(np.float64)
    rnd = rng.normal(size=(N, 3))
    if s.D == 2:
        rnd[:, 2] = 0
    # in the primitive's plane: cross(n, e_k); the axis the normal is closest to gives no direction, so k avoids it
    k = (np.argmax(np.abs(n), axis=1) + rng.integers(1, 3, N)) % 3
    if s.D == 2:
        k[:] = 2
    inplane = np.cross(n, np.eye(3)[k])
    mirror = din - 2.0 * np.sum(din * n, axis=1, keepdims=True) * n
    kind = np.arange(N) % 3
    d = np.where((kind == 0)[:, None], rnd, np.where((kind == 1)[:, None], inplane, mirror))
    return o, _unit32(s, d)


def _far(s, fams):
    """the `rim` (and `vertex_edge`) rays with the origin moved back along -d by 64 times the scene's largest coordinate, in
    float32 arithmetic: the slab tests round o * inv at the magnitude of the origin"""
    if "vertex_edge" in fams:
        o = np.concatenate([fams["rim"][0][: N // 2], fams["vertex_edge"][0][: N - N // 2]])
        d = np.concatenate([fams["rim"][1][: N // 2], fams["vertex_edge"][1][: N - N // 2]])
    else:
        o, d = fams["rim"]
    back = np.float32(64) * np.float32(max(np.abs(s.lo).max(), np.abs(s.hi).max()))
    return (o - d * back).astype(np.float32), d.copy()


def families(scene, rng_seed):
    """{name: (origins f32[N,3], directions f32[N,3])} for a Scene; deterministic in rng_seed"""
    s = scene
    seeds = np.random.SeedSequence(rng_seed).spawn(8)
    rngs = [np.random.default_rng(q) for q in seeds]
    out = {}
    out["axis"] = _finish(s, *_axis(s, rngs[0]))
    out["graze"] = _finish(s, *_graze(s, rngs[1]))
    out["rim"] = _finish(s, *_rim(s, rngs[2]))
    out["tiny"] = _finish(s, *_tiny(s, rngs[3]))
    out["wall_edge"] = _finish(s, *_wall_edge(s, rngs[4]))
    if s.verts is not None:
        out["vertex_edge"] = _finish(s, *_vertex_edge(s, rngs[5]))
    out["restart"] = _finish(s, *_restart(s, rngs[6], out))
    out["far"] = _finish(s, *_far(s, out))
    return out


SEED = 20240


@functools.lru_cache(maxsize=None)
def scene_families(name):
    return families(scene(name), SEED)


@functools.lru_cache(maxsize=None)
def reference(name, family):
    """brute-force answer of the oracle for one scene x family cell (computed once, shared by the tests, never changed)"""
    o, d = scene_families(name)[family]
    g, p, t = brute_force(scene(name), o, d)
    for a in (g, p, t):
        a.setflags(write=False)
    return g, p, t


def bvh_walk(name, family):
    o, d = scene_families(name)[family]
    return _intersect(scene(name).oracle, o, d, False)


# Rays that exposed a fault, kept by value: name -> (scene, origin, direction, geomID, primID, t), floats in hex.
#   far_tie_*: from 64 scene sizes away two overlapping disks of one plane are met at the SAME t; the lower original id
#   wins.  Both per-lane walks compared a box's entry bound with the closest hit so far without allowance for the bound's
#   own rounding (a few ulp of the distance): the box of the lower id, visited second, was culled when its bound came out
#   an ulp above that t, and the higher id was returned (VR_SLAB_SLACK, vr_walk.hpp).
KNOWN_ANSWERS = {
    "far_tie_plane": ("plane", ("-0x1.2a2dbcp+5", "-0x1.67c5b8p+7", "0x1.61f1eep+10"),
                      ("0x1.2f9e92p-6", "0x1.e3ee74p-4", "-0x1.fc5350p-1"), 1, 2002, "0x1.6480eep+10"),
    "far_tie_coincident_a": ("coincident", ("-0x1.7852bcp+7", "0x1.8243acp+7", "0x1.1cfc08p+9"),
                             ("0x1.2ac43ap-2", "-0x1.2cfd22p-2", "-0x1.d2069ep-1"), 1, 358, "0x1.391940p+9"),
    "far_tie_coincident_b": ("coincident", ("0x1.3571fap+7", "0x1.d9f74ap+2", "0x1.2e4aacp+9"),
                             ("-0x1.09dc8cp-2", "-0x1.ef09fep-8", "-0x1.ee6d6ap-1"), 1, 145, "0x1.390918p+9"),
}


def known_answer(name):
    """(origin f32[1,3], direction f32[1,3], (geomID, primID, t) arrays as recorded)"""
    _, o, d, geom, prim, t = KNOWN_ANSWERS[name]
    o = np.array([[float.fromhex(x) for x in o]], dtype=np.float32)
    d = np.array([[float.fromhex(x) for x in d]], dtype=np.float32)
    return o, d, (np.array([geom], np.int32), np.array([prim], np.uint32), np.array([float.fromhex(t)], np.float32))


def hexray(o, d):
    return "o=(%s) d=(%s)" % (", ".join(float(x).hex() for x in o), ", ".join(float(x).hex() for x in d))
