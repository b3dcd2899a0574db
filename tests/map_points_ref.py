"""Brute-force float64 reference of vr_map_to_points* (include/viennaray_amd.h has the definition): all m x n distances.

    d_ij = |p_i - c_j|, in range iff d_ij < R, w_ij = (1 - d_ij / R) * g_ij, g_ij = 1 or max(0, n_j . m^_i);
    out[i] = sum w f / sum w if sum w > 0, else f[j*], j* the nearest centre (lowest id on a tie).

Per query it also reports what a comparison needs to know about the query's conditioning:
    K          the in-range count
    sum_w      the sum of weights
    gap        (second smallest - smallest squared centre distance) / smallest (inf where the smallest is 0 or n == 1)
    ambiguous  some centre has |d - R| < 1e-5 R (in range or not is a matter of float32 rounding), or 0 < sum_w < 0.05
               (the mean is the quotient of two tiny sums)
For nearest-only checks a query is also ambiguous if gap < 1e-4 (ambiguous_nearest).
Ambiguous queries are left out of value comparisons; MAX_AMBIGUOUS caps their share in every test that leaves any out.
"""
import numpy as np

MAX_AMBIGUOUS = 0.02
EPS = 2.0 ** -23


def triangle_centroids(verts, tris):
    """((v0 + v1) + v2) * (1.f / 3.f) per component, in float32: the centre the library uses for a triangle"""
    v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(tris).astype(np.int64).reshape(-1, 3)
    return ((v[t[:, 0]] + v[t[:, 1]]) + v[t[:, 2]]) * np.float32(1.0 / 3.0)


def triangle_normals(verts, tris):
    """unit normals in float64 (the library's float32 ones differ from them by rounding)"""
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    t = np.ascontiguousarray(tris).astype(np.int64).reshape(-1, 3)
    n = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
    return n / np.linalg.norm(n, axis=1)[:, None]


def reference(values, centres, prim_normals, points, query_normals, radius, D=3, chunk=512):
    """dict of out, jstar, K, sum_w, gap, ambiguous, ambiguous_nearest (arrays of m).  Rows with a coordinate that is
    not finite give out = NaN, jstar = -1 and are never ambiguous."""
    f = np.asarray(values, dtype=np.float64).reshape(-1)
    c = np.asarray(centres, dtype=np.float64).reshape(-1, 3)[:, :D]
    p = np.asarray(points, dtype=np.float64)
    p = p.reshape(-1, p.shape[-1])[:, :D]
    n, m, R = c.shape[0], p.shape[0], float(radius)
    gate = query_normals is not None
    if gate:
        nj = np.asarray(prim_normals, dtype=np.float64).reshape(-1, 3)[:, :D]
        q = np.asarray(query_normals, dtype=np.float64)
        q = q.reshape(-1, q.shape[-1])[:, :D]
        q = q / np.linalg.norm(q, axis=1)[:, None]
    out = np.empty(m)
    jstar = np.empty(m, dtype=np.int64)
    K = np.empty(m, dtype=np.int64)
    sum_w = np.empty(m)
    gap = np.empty(m)
    amb = np.empty(m, dtype=bool)
    for lo in range(0, m, chunk):
        hi = min(m, lo + chunk)
        d2 = ((p[lo:hi, None, :] - c[None, :, :]) ** 2).sum(axis=2)
        d = np.sqrt(d2)
        js = np.argmin(d2, axis=1)  # (the first minimum: the lowest id on a tie)
        d2min = d2[np.arange(hi - lo), js]
        if n > 1:
            second = np.partition(d2, 1, axis=1)[:, 1]
            with np.errstate(divide="ignore", invalid="ignore"):
                g = np.where(d2min > 0, (second - d2min) / d2min, np.inf)
        else:
            g = np.full(hi - lo, np.inf)
        inr = d < R
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.where(inr, 1.0 - d / R, 0.0) if R > 0 else np.zeros_like(d)
        if gate:
            w = w * np.maximum(0.0, q[lo:hi] @ nj.T)
        sw = w.sum(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            mean = (w * f[None, :]).sum(axis=1) / sw
        out[lo:hi] = np.where(sw > 0, mean, f[js])
        jstar[lo:hi] = js
        K[lo:hi] = inr.sum(axis=1)
        sum_w[lo:hi] = sw
        gap[lo:hi] = g
        amb[lo:hi] = (np.abs(d - R) < 1e-5 * R).any(axis=1) | ((sw > 0) & (sw < 0.05))
    bad = ~np.isfinite(p).all(axis=1)
    out[bad] = np.nan
    jstar[bad] = -1
    amb[bad] = False
    gap[bad] = np.inf
    return dict(out=out, jstar=jstar, K=K, sum_w=sum_w, gap=gap, ambiguous=amb, ambiguous_nearest=amb | (gap < 1e-4))


def tolerance(ref, values):
    """|out - ref| <= (K + 8) * 2^-23 * max|values| / min(1, sum_w): float32 rounding of the K weights and of the two sums
    of non-negative terms, relative to the sum of weights where that is below one.  Where the mean does not apply
    (sum_w == 0: the nearest centre's value) the result is exact: tolerance 0."""
    vmax = float(np.max(np.abs(np.asarray(values, dtype=np.float64))))
    sw = ref["sum_w"]
    with np.errstate(divide="ignore"):
        tol = (ref["K"] + 8) * EPS * vmax / np.minimum(1.0, sw)
    return np.where(sw > 0, tol, 0.0)
