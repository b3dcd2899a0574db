"""Closed-form flux references that do not go through the oracle, and the scenes they hold for.

One scene, three descriptions of it: a rectangular trench (width w, depth d, flat top out to |x| = L) as a triangle
mesh extruded along y, as a 3-D disk cloud and as a 2-D disk row.  The profile is a convex rectangle, so no two points
of its interior occlude each other and the flux a surface element receives has a closed form:

  radiosity(w, d, s)              diffuse particles of sticking s: the 2-D cosine-law radiosity system
  specular_bottom(w, d, s, x)     specular particles: mirror images of the opening in the two side walls
  power_cosine_bottom(w, d, n, x) sticking 1 under a cos^n source: the in-plane angle integral

Everything here is float64 numpy.  This module imports neither the oracle nor the tracing library: the scenes are plain
arrays, the references plain formulas, and both test files (tests/test_closed_form_flux_host.py: the oracle;
tests/test_closed_form_flux.py: the device) go through the same builders, cases and tolerances below.

A "row" is one cell of the profile: (part, coordinate), with part one of TOP / BOTTOM / LEFT / RIGHT and the coordinate
the x (top, bottom) or z (walls) of the cell centre.  A row's measured value is the mean over y of the SOURCE-normalised
flux of its primitives; its reference value is the mean of the closed form over the row's footprint (the unit cell of
a mesh row, centre +- r of a disk row).
"""
import functools
import math
from collections import namedtuple

import numpy as np

TOP, BOTTOM, LEFT, RIGHT = 0, 1, 2, 3
PART_NAMES = {TOP: "top", BOTTOM: "bottom", LEFT: "left wall", RIGHT: "right wall"}
REFLECTIVE, PERIODIC = 0, 1      # rayBoundary.hpp:10-14 (the values of both front ends)
POS_Y = 2                        # rayUtil.hpp:40-47

W, DEPTH, L, NY = 10, 10, 10, 8  # the scene of every case


# ---------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------
Mesh = namedtuple("Mesh", "verts tris part coord")
Disks = namedtuple("Disks", "points normals part coord radius D")


def trench_mesh(w=W, d=DEPTH, L=L, ny=NY):
    """Unit quads of two triangles each, wound so that cross(v1 - v0, v2 - v0) faces the open side: top strips at z = 0
    for w/2 < |x| < L, the bottom at z = -d, walls at x = -+w/2; y runs over [0, ny]."""
    assert w % 2 == 0, "the walls lie on grid lines"
    verts, tris, part, coord = [], [], [], []

    def quad(o, e1, e2, p, c):
        o, e1, e2 = (np.asarray(a, dtype=np.float64) for a in (o, e1, e2))
        k = len(verts)
        verts.extend([o, o + e1, o + e1 + e2, o + e2])
        tris.extend([(k, k + 1, k + 2), (k, k + 2, k + 3)])
        part.extend([p, p])
        coord.extend([c, c])

    ex, ey, ez = (1, 0, 0), (0, 1, 0), (0, 0, 1)
    for j in range(ny):
        for i in range(-L, L):
            if i >= w // 2 or i < -w // 2:
                quad((i, j, 0), ex, ey, TOP, i + 0.5)
        for i in range(-w // 2, w // 2):
            quad((i, j, -d), ex, ey, BOTTOM, i + 0.5)
        for k in range(d):
            quad((-w / 2, j, -k - 1), ey, ez, LEFT, -k - 0.5)    # ey x ez = +x
            quad((w / 2, j, -k - 1), ez, ey, RIGHT, -k - 0.5)    # ez x ey = -x
    return Mesh(np.asarray(verts, dtype=np.float32), np.asarray(tris, dtype=np.uint32),
                np.asarray(part), np.asarray(coord, dtype=np.float64))


def triangle_centroids(mesh):
    """centroid and (unnormalised) normal of every triangle, float64"""
    a, b, c = (mesh.verts[mesh.tris[:, k]].astype(np.float64) for k in range(3))
    return (a + b + c) / 3.0, np.cross(b - a, c - a)


def disk_radius(D, grid_delta=1.0):
    """the radius the tracer reports (rayUtil.hpp:99-101; DISK_FACTOR_3D / _2D of tests/helpers.py)"""
    return 0.5 * (1.7320508 if D == 3 else 1.41421356237) * (1 + 1e-5) * grid_delta


def trench_disks(D, w=W, d=DEPTH, L=L, ny=NY, overhang=False):
    """The profile of trench_mesh as a disk cloud of gridDelta 1 in which no disk overhangs the opening: the first top
    centre at |x| = w/2 + r, the first wall centre at z = -r, then steps of 1 (the last wall centre is the first whose
    footprint reaches below -d); bottom centres on the cell centres.  D == 3: rows at y = 0 .. ny (the walls of the
    periodic y direction go through the first and last centres, as in the reference's grids).  D == 2: one row in the
    xy plane with y up (setSourceDirection(POS_Y)).

    overhang=True is the regular layout instead (top centres on the cell centres, so that the first top disk overhangs
    the opening by r - 1/2): only for the figure in DESIGN.md."""
    r = disk_radius(D)
    prof = []    # (x, z, nx, nz, part, coord)
    first = w / 2 + (0.5 if overhang else r)
    for k in range(int(math.floor(L - first)) + 1):
        for sgn in (-1, 1):
            prof.append((sgn * (first + k), 0.0, 0.0, 1.0, TOP, sgn * (first + k)))
    for i in range(w):
        prof.append((-w / 2 + i + 0.5, -d, 0.0, 1.0, BOTTOM, -w / 2 + i + 0.5))
    for k in range(d):
        z = -(0.5 if overhang else r) - k
        prof.append((-w / 2, z, 1.0, 0.0, LEFT, z))
        prof.append((w / 2, z, -1.0, 0.0, RIGHT, z))
    prof = np.asarray(prof, dtype=np.float64)
    rows = range(ny + 1) if D == 3 else [0]
    pts, nrm, part, coord = [], [], [], []
    for j in rows:
        for x, z, nx, nz, p, c in prof:
            pts.append((x, j, z) if D == 3 else (x, z, 0.0))
            nrm.append((nx, 0.0, nz) if D == 3 else (nx, nz, 0.0))
            part.append(int(p))
            coord.append(c)
    return Disks(np.asarray(pts, dtype=np.float32), np.asarray(nrm, dtype=np.float32), np.asarray(part),
                 np.asarray(coord, dtype=np.float64), r, D)


def rows_of(part, coord):
    """[(part, coord, indices)] of the distinct rows, in a fixed order"""
    out = []
    for p in (TOP, BOTTOM, LEFT, RIGHT):
        for c in np.unique(coord[part == p]):
            out.append((p, float(c), np.nonzero((part == p) & (coord == c))[0]))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------
def _view(p, n, a, b):
    """Fraction of the 2-D cosine-law emission of a point p (normal n) that lands on the segment [a, b]: the kernel
    max(0, n.r^) max(0, -n'.r^) / (2 |r|) integrated exactly over the segment, 1/2 |sin(t_b) - sin(t_a)| with t the
    angle from the normal.  By reciprocity also the flux density at p from a unit-radiosity emitter [a, b].  Every
    pair of points of a convex profile sees each other, so nothing is clipped; broadcasting over leading axes."""
    t = np.stack([n[..., 1], -n[..., 0]], axis=-1)

    def sin_from_normal(q):
        r = q - p
        return (r * t).sum(-1) / np.sqrt((r * r).sum(-1))

    return 0.5 * np.abs(sin_from_normal(b) - sin_from_normal(a))


class Radiosity:
    """the solved system of radiosity(): per segment its part, interval [lo, hi] of the profile coordinate, the direct
    flux F_direct and the total incoming flux F"""

    def __init__(self, w, d, s, m, scallop=None):
        self.w, self.d, self.s, self.m = w, d, s, m
        h = 1.0 / m
        e = np.arange(m * d) * h                     # walls: coordinate z from 0 downwards
        eb = -w / 2 + np.arange(m * w) * h           # bottom: coordinate x
        z = np.zeros_like
        segs = [  # part, a (x, z), b (x, z), normal, lo, hi
            (LEFT, np.stack([z(e) - w / 2, -e - h], 1), np.stack([z(e) - w / 2, -e], 1), (1.0, 0.0), -e - h, -e),
            (BOTTOM, np.stack([eb, z(eb) - d], 1), np.stack([eb + h, z(eb) - d], 1), (0.0, 1.0), eb, eb + h),
            (RIGHT, np.stack([z(e) + w / 2, -e - h], 1), np.stack([z(e) + w / 2, -e], 1), (-1.0, 0.0), -e - h, -e)]
        self.part = np.concatenate([np.full(len(s_[1]), s_[0]) for s_ in segs])
        self.a = np.concatenate([s_[1] for s_ in segs])
        self.b = np.concatenate([s_[2] for s_ in segs])
        self.n = np.concatenate([np.tile(np.asarray(s_[3]), (len(s_[1]), 1)) for s_ in segs])
        self.lo = np.concatenate([s_[4] for s_ in segs])
        self.hi = np.concatenate([s_[5] for s_ in segs])
        self.mid = 0.5 * (self.a + self.b)
        self.open_a, self.open_b = np.array([-w / 2, 0.0]), np.array([w / 2, 0.0])
        self.F_direct = _view(self.mid, self.n, self.open_a, self.open_b)
        if scallop is not None:
            for a, b, seen_by in scallop_emitters(w, *scallop):
                self.F_direct = self.F_direct + _view(self.mid, self.n, a, b) * np.isin(self.part, seen_by)
        K =_view(self.mid[:, None, :], self.n[:, None, :], self.a[None, :, :], self.b[None, :, :])
        K[self.part[:, None] == self.part[None, :]] = 0.0     # a flat part does not see itself
        self.K = K
        rho = np.full(len(K), 1.0 - s)
        if scallop is not None:     # the top g of either wall is a gap: nothing is reflected from there
            rho = rho * (1.0 - np.clip(self.hi + scallop[0], 0.0, h) / h * (self.part != BOTTOM))
        self.F = np.linalg.solve(np.eye(len(K)) - K * rho[None, :], self.F_direct)

    def _mean(self, values, part, lo, hi):
        if part == TOP:
            return 1.0
        ov = np.clip(np.minimum(self.hi, hi) - np.maximum(self.lo, lo), 0.0, None) * (self.part == part)
        return float((ov * values).sum() / ov.sum())

    def row_mean(self, part, lo, hi):
        """mean of F over [lo, hi] of the part's coordinate (clipped to the part); the top surface is 1"""
        return self._mean(self.F, part, lo, hi)

    def direct_at(self, part, coord):
        """F_direct at single points of the profile (part, coordinate): exact, no discretisation"""
        part, coord = np.asarray(part), np.asarray(coord, dtype=np.float64)
        w, d = self.w, self.d
        p = np.where((part == BOTTOM)[:, None], np.stack([coord, np.full_like(coord, -d)], 1),
                     np.stack([np.where(part == LEFT, -w / 2, w / 2), coord], 1))
        n = np.where((part == BOTTOM)[:, None], (0.0, 1.0),
                     np.stack([np.where(part == LEFT, 1.0, -1.0), np.zeros_like(coord)], 1))
        return _view(p, n, self.open_a, self.open_b), p, n

    def second_term(self):
        """K @ F_direct: the second term of the Neumann series, on this discretisation"""
        return self.K @ self.F_direct

    def from_emitters(self, part, coord, strength):
        """The same term for emitters that are points of the profile (lines along y): emitter q sends `strength[q]`
        (radiosity times the length it stands for) along the cosine law about its normal.  Returns per segment the
        arriving flux density, and per segment sum_q strength^2 * view / length (for the variance of a Monte-Carlo
        estimate with equal rays per emitter)."""
        _, p, n = self.direct_at(part, coord)
        V = _view(p[None, :, :], n[None, :, :], self.a[:, None, :], self.b[:, None, :])    # [segment, emitter]
        V[self.part[:, None] == np.asarray(part)[None, :]] = 0.0
        length = 1.0 / self.m
        return V @ strength / length, V, length


def scallop_depth(r):
    """Mean depth of the gaps that unit-spaced discs of radius r leave along a straight edge of the surface they cover:
    at offset t from a centre the cover ends sqrt(r^2 - t^2) from the row of centres, not r; the mean of the difference
    over t in [-1/2, 1/2].  0.0509 for r = DISK_FACTOR_3D."""
    return r - (0.5 * math.sqrt(r * r - 0.25) + r * r * math.asin(0.5 / r))


def scallop_emitters(w, g, X):
    """What the scalloped edges of a 3-D disk cloud add to the trench's direct flux (trench_disks(3); g =
    scallop_depth(r), X = the reflective wall of the domain in x).

    The discs end in round scallops at the two convex corners: the rim of the top surface stops short of |x| = w/2 by g
    on the average over y, and so does the top of each wall short of z = 0.  A disc lets a ray through from behind
    once (rayTraceKernel.hpp: hitFromBack), so the space behind a wall is not closed to such rays:
      - a ray through a rim gap that heads inwards crosses the wall from behind and lands in the trench as if the
        opening were wider by g on that side;
      - one that heads outwards is reflected at the domain wall x = +-X, comes back and crosses the wall from behind
        (unless it has left through the open bottom of the domain by then): the mirror image of the rim gap in x = X;
      - a ray from the opening that leaves the trench through the gap at the top of a wall does the same: seen from
        inside, the mirror image of that gap shows the mirror image of the opening behind it.
    Each is a segment that looks like the opening (radiosity 1) from wherever it can be seen: the bottom sees all six,
    a wall the three of the opposite side.  In two dimensions (trench_disks(2)) discs are segments that end where they
    should, and none of this exists.  [(a, b, parts that see it)]"""
    out = []
    for sgn, wall in ((1.0, LEFT), (-1.0, RIGHT)):      # the emitters on the side x = sgn * w/2, seen by `wall`
        e, far = sgn * w / 2, sgn * (2 * X - w / 2)
        out.append((np.array([e, 0.0]), np.array([e + sgn * g, 0.0]), (BOTTOM, wall)))
        out.append((np.array([far - sgn * g, 0.0]), np.array([far, 0.0]), (BOTTOM, wall)))
        out.append((np.array([far, -g]), np.array([far, 0.0]), (BOTTOM, wall)))
    return out


@functools.lru_cache(maxsize=None)
def radiosity(w=W, d=DEPTH, s=1.0, m=40, scallop=None):
    """The trench interior cut into segments of length 1/m (both walls and the bottom) under the opening as an emitter
    of radiosity 1, with the 2-D cosine-law kernel — what 3-D Lambert emission integrates to along an extrusion, and
    what the D = 2 diffuse reflection samples.  F_direct = K . opening, (I - (1 - s) K) F = F_direct; F is the INCOMING
    weight per unit length (what DiffuseParticle::surfaceCollision credits), not that weight times the sticking.
    K is integrated exactly over the emitting segment and collocated at the receiving segment's midpoint.
    scallop = (g, X) adds scallop_emitters(w, g, X) to F_direct (3-D disk clouds only)."""
    return Radiosity(w, d, s, m, scallop)


_GL_X, _GL_W = np.polynomial.legendre.leggauss(64)


def _cell_mean(f, lo, hi):
    x = 0.5 * (lo + hi) + 0.5 * (hi - lo) * _GL_X
    return float((f(x) * _GL_W).sum() / 2.0)


def specular_bottom(w, d, s, x, kmax=200):
    """Bottom flux under specular reflection with sticking s and a power-1 source: the opening and its mirror images
    [a_k, b_k] = [-w/2 + k w, w/2 + k w] in the side walls, image k through |k| reflections of weight (1 - s) each.
    A specular ray that leaves the flat bottom goes up and never comes back, so the bottom needs nothing else."""
    x = np.asarray(x, dtype=np.float64)
    f = np.zeros_like(x)
    for k in range(-kmax, kmax + 1):
        a, b = -w / 2 + k * w, w / 2 + k * w
        f += (1.0 - s) ** abs(k) * 0.5 * ((b - x) / np.hypot(b - x, d) - (a - x) / np.hypot(a - x, d))
    return f


def power_cosine_bottom(w, d, n, x):
    """Bottom flux at sticking 1 under a source of pdf ~ cos^n(theta) per solid angle, relative to the flat-surface
    flux: int_{phi1}^{phi2} cos^n(phi) dphi / int_{-pi/2}^{pi/2} cos^n(phi) dphi with phi the in-plane angle to the
    opening's edges (the out-of-plane integral is the same factor above and below)."""
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    p1, p2 = np.arctan2(-w / 2 - x, d), np.arctan2(w / 2 - x, d)
    gx, gw = np.polynomial.legendre.leggauss(200)
    phi = 0.5 * (p1 + p2)[:, None] + 0.5 * (p2 - p1)[:, None] * gx[None, :]
    num = (np.cos(phi) ** n * gw[None, :]).sum(1) * 0.5 * (p2 - p1)
    den = math.sqrt(math.pi) * math.gamma((n + 1) / 2.0) / math.gamma(n / 2.0 + 1.0)
    return num / den




# ---------------------------------------------------------------------------------------------------------------------
# cases, rows and tolerances (shared by the host and the device test)
# ---------------------------------------------------------------------------------------------------------------------
DIFFUSE, SPECULAR = "diffuse", "specular"
Case = namedtuple("Case", "id scene particle sticking power bcx reference")

CASES = [
    Case("mesh-diffuse-1.0", "mesh", DIFFUSE, 1.0, 1.0, REFLECTIVE, "radiosity"),
    Case("mesh-diffuse-0.2", "mesh", DIFFUSE, 0.2, 1.0, REFLECTIVE, "radiosity"),
    Case("mesh-specular-0.3", "mesh", SPECULAR, 0.3, 1.0, REFLECTIVE, "images"),
    Case("mesh-specular-1.0-power-8", "mesh", SPECULAR, 1.0, 8.0, REFLECTIVE, "power"),
    Case("mesh-specular-1.0-power-50", "mesh", SPECULAR, 1.0, 50.0, REFLECTIVE, "power"),
    Case("mesh-diffuse-0.2-periodic-x", "mesh", DIFFUSE, 0.2, 1.0, PERIODIC, "radiosity"),
    Case("disks3-diffuse-1.0", "disks3", DIFFUSE, 1.0, 1.0, REFLECTIVE, "radiosity"),
    Case("disks3-diffuse-0.2", "disks3", DIFFUSE, 0.2, 1.0, REFLECTIVE, "radiosity"),
    Case("disks2-diffuse-1.0", "disks2", DIFFUSE, 1.0, 1.0, REFLECTIVE, "radiosity"),
    Case("disks2-diffuse-0.2", "disks2", DIFFUSE, 0.2, 1.0, REFLECTIVE, "radiosity"),
]
CASE_IDS = [c.id for c in CASES]

HOST_RAYS = 2_000_000
GPU_RAYS = 20_000_000
SEED = 7
SCATTER_SEEDS = tuple(range(101, 109))

# Row-wise scatter of the ORACLE over the 8 seeds SCATTER_SEEDS at HOST_RAYS, for the cases with sticking < 1 (their
# credits are weighted and correlated, so there is no clean binomial bound): per case and part the largest relative
# standard deviation (ddof = 1) of a compared row.  Produced on the CPU by
#     python tests/test_closed_form_flux_host.py scatter
# The tolerance of such a row is 5 x scatter + 2e-3 at HOST_RAYS; the device test evaluates the same formula with the
# scatter scaled by sqrt(HOST_RAYS / GPU_RAYS).  Never re-measured from device output.
SCATTER = {
    "mesh-diffuse-0.2": {"top": 0.00070, "bottom": 0.00369, "wall": 0.00598},
    "mesh-specular-0.3": {"bottom": 0.00365},
    "mesh-diffuse-0.2-periodic-x": {"top": 0.00070, "bottom": 0.00380, "wall": 0.00608},
    "disks3-diffuse-0.2": {"top": 0.00110, "bottom": 0.00285, "wall": 0.00532},
    "disks2-diffuse-0.2": {"top": 0.00048, "bottom": 0.00378, "wall": 0.00379},
}
# The systematic offset of the 3-D disk cloud against the plain rectangle: the mean over the compared rows of what
# scallop_emitters() and the missing reflection from the top of the walls add to the reference, by sticking and part.
# Without them the oracle reads this much high (the bottom: +0.8 ... +2.0 % per row at HOST_RAYS, against a noise of
# ~0.5 %); with them its mean over the 8 seeds is within 0.2 % of the reference on every bottom row.  The cause and
# its derivation: scallop_emitters.  A record, checked by the host test against the references themselves; no
# tolerance is widened by it.
DISK3_SCALLOP_OFFSET = {1.0: {"bottom": 0.0139, "wall": 0.0085}, 0.2: {"bottom": 0.0093, "wall": 0.0059}}
REFERENCE_ERROR = 2e-3   # the reference's own discretisation (m = 40 against m = 80 is bounded at half of this)

Row = namedtuple("Row", "label key part coord idx ref expected_credits")
Scene = namedtuple("Scene", "kind D geom bcs source_direction source_area rows excluded")


def disk_excluded(disks, w=W, d=DEPTH):
    """The rows of a disk cloud whose footprint reaches a concave corner, where the neighbouring part hides a part of
    the disc: the two outermost bottom rows and the deepest wall row (the same row of the profile on either wall).
    Named here, not found by a threshold; every other row is compared."""
    deepest = float(np.min(disks.coord[disks.part == LEFT]))
    assert deepest - disks.radius < -d <= deepest + disks.radius
    return [(BOTTOM, -(w - 1) / 2.0), (BOTTOM, (w - 1) / 2.0), (LEFT, deepest), (RIGHT, deepest)]


def _credit_efficiency(r):
    """A ray that lands in the strip of a row of unit-spaced 3-D discs is credited to every disc that contains the
    point (0, 1 or 2 of the row): (E m)^2 / E m^2 over the strip is the factor by which the row's mean is noisier than
    a plain count of the rays in the strip."""
    u, y = np.meshgrid((np.arange(400) + 0.5) / 400 * 2 * r - r, (np.arange(400) + 0.5) / 400)
    m = sum(((u * u + (y - j) ** 2) < r * r).astype(np.float64) for j in (-1, 0, 1, 2))
    return float(m.mean() ** 2 / (m * m).mean())


@functools.lru_cache(maxsize=None)
def scene_of(case_id):
    """geometry, settings and the compared rows (with their reference values) of a case"""
    case = CASES[CASE_IDS.index(case_id)]
    w, d, ny = W, DEPTH, NY
    if case.scene == "mesh":
        g, D, half, excluded = trench_mesh(), 3, 0.5, []
        bcs, direction = [case.bcx, PERIODIC, REFLECTIVE], None
        source_area, row_area, eff, scallop = 2.0 * L * ny, 1.0 * ny, 1.0, None
    else:
        D = 3 if case.scene == "disks3" else 2
        g = trench_disks(D)
        half, excluded = g.radius, disk_excluded(g)
        xs = g.points[:, 0].astype(np.float64)
        width = xs.max() - xs.min()          # the tracer's bounding box is that of the centres
        if D == 3:
            bcs, direction = [case.bcx, PERIODIC, REFLECTIVE], None
            source_area, row_area, eff = width * ny, 2 * g.radius * ny, _credit_efficiency(g.radius)
            scallop = (scallop_depth(g.radius), float(xs.max()))
        else:
            bcs, direction = [REFLECTIVE, REFLECTIVE], POS_Y
            source_area, row_area, eff, scallop = width, 2 * g.radius, 1.0, None

    if case.reference == "radiosity":
        R = radiosity(w, d, case.sticking, 40, scallop)
        parts = (BOTTOM, LEFT, RIGHT)

        def ref_of(p, c):
            return R.row_mean(p, c - half, c + half)
    else:
        parts = (BOTTOM,)

        def bottom(x):
            if case.reference == "images":
                return specular_bottom(w, d, case.sticking, x)
            return power_cosine_bottom(w, d, case.power, x)

        def ref_of(p, c):
            return _cell_mean(bottom, c - half, c + half)

    rows = []
    if case.reference == "radiosity":      # the top surface as one row: its mean is 1
        idx = np.nonzero(g.part == TOP)[0]
        cells = len(np.unique(g.coord[idx]))
        cell_area = ny if D == 3 else 1.0      # (centres a unit apart: the discs' strips overlap, the cells do not)
        rows.append(Row("top mean", "top", TOP, float("nan"), idx, 1.0, cells * cell_area * eff / source_area))
    for p, c, idx in rows_of(g.part, g.coord):
        if p in parts and (p, c) not in excluded:
            ref = ref_of(p, c)
            rows.append(Row("%s %+.3f" % (PART_NAMES[p], c), "bottom" if p == BOTTOM else "wall", p, c, idx, ref,
                            ref * row_area * eff / source_area))
    return Scene("mesh" if case.scene == "mesh" else "disks", D, g, bcs, direction, source_area, rows, excluded)


def tolerance(case, row, num_rays):
    """Sticking 1: a row's credits are binomial with expectation E = N F_ref A_row / A_source (times the crediting
    efficiency of overlapping discs), and the bound is 5 / sqrt(E).  Sticking < 1: 5 x the recorded scatter of the
    oracle, scaled from HOST_RAYS by 1 / sqrt(N).  Both plus the reference's own error."""
    if case.sticking == 1.0:
        return 5.0 / math.sqrt(num_rays * row.expected_credits) + REFERENCE_ERROR
    return 5.0 * SCATTER[case.id][row.key] * math.sqrt(HOST_RAYS / num_rays) + REFERENCE_ERROR


def compare(case_id, flux, num_rays, who):
    """`flux`: the SOURCE-normalised flux per primitive.  Returns (report, failures, worst): the report one line per
    row, the failures a list of lines, worst = (fraction of its bound used, row label) of the worst row."""
    case = CASES[CASE_IDS.index(case_id)]
    flux = np.asarray(flux, dtype=np.float64)
    report, failures, worst = [], [], (0.0, "")
    for row in scene_of(case_id).rows:
        got = float(flux[row.idx].mean())
        tol = tolerance(case, row, num_rays)
        err = got / row.ref - 1.0
        line = "%s %s: %-18s got %.5f ref %.5f rel %+.4f bound %.4f (%.0f %% of it)" % (
            who, case_id, row.label, got, row.ref, err, tol, 100 * abs(err) / tol)
        report.append(line)
        if not abs(err) <= tol:
            failures.append(line)
        if abs(err) / tol > worst[0]:
            worst = (abs(err) / tol, row.label)
    report.append("%s %s: worst row '%s' uses %.0f %% of its bound" % (who, case_id, worst[1], 100 * worst[0]))
    return report, failures, worst
