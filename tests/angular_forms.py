"""Closed forms of the angular gather (Trace.gatherAngular) on the trench of tests/closed_forms.py, as quadratures.

Derived from neither the oracle nor the library: float64 numpy, Gauss-Legendre nodes, the laws as the piecewise-linear
functions of a cosine the definition says they are (np.interp over the nodes k / (M - 1)).  With
    omega = (sin(phi) cos(psi), sin(psi), cos(phi) cos(psi)),   d omega = cos(psi) d psi d phi
phi is the angle in the profile's plane from the source axis z and psi the elevation along the extrusion y, over which
the trench does not change: what a point sees is a range of phi, for every psi in (-pi/2, pi/2).

A gather sample leaves primitive i along the cosine law about its normal m (density m . omega / pi) and, if it reaches
the source, weighs g_L L(c) T Y(m . omega) with g_L = pi / Z.  Its expectation is
    F_i = (1 / Z) int_visible L(c) T(omega) Y(m . omega) (m . omega) d omega,     Z = 2 pi int_0^1 L(c) c dc  (pi for L = 1).
In 2-D the density is cos(phi) / 2 and g_L = 2 / Z_2 with Z_2 = int_{-pi/2}^{pi/2} L(cos phi) cos(phi) d phi.

  source_bottom(table, x)        sticking 1: (1 / Z) iint L(cos phi cos psi) cos(phi) cos^2(psi) d psi d phi over the opening
  source_bottom_2d(table, x)     the 2-D trench: int L(cos phi) cos(phi) d phi / Z_2
  yield_wall(table, z)           power-1 source, sticking 1, a wall point at height z < 0: m . omega = sin(phi) cos(psi), NOT c:
                                 (1 / pi) iint Y(sin phi cos psi) sin(phi) cos^2(psi) d psi d phi, phi in [0, atan(w / |z|)]
  reflectivity_bottom(table, rho, x)
                                 SPECULAR, a power-1 source: the mirror images of the opening (closed_forms.specular_bottom);
                                 a mirror keeps |omega_x|, so each of the |k| wall bounces of a ray towards image k has the same
                                 mu = |sin phi| cos psi, and the ray brings back (rho R(mu))^|k|
Every function takes the number of nodes per axis; converged() runs it at n and 2 n and returns the finer value with the
largest difference between the two, which the tests bound by 1e-6 on the CPU."""
import numpy as np

W, DEPTH = 10, 10  # closed_forms.W, closed_forms.DEPTH


def law(table, x):
    """the piecewise-linear function of a cosine x in [0, 1] a table stands for, float64"""
    t = np.asarray(table, dtype=np.float64)
    return np.interp(np.clip(x, 0.0, 1.0), np.linspace(0.0, 1.0, len(t)), t)


def _gl(n, lo, hi):
    """Gauss-Legendre nodes and weights on [lo, hi] (arrays broadcast over a leading axis of intervals)"""
    x, w = np.polynomial.legendre.leggauss(n)
    lo, hi = np.asarray(lo, dtype=np.float64)[..., None], np.asarray(hi, dtype=np.float64)[..., None]
    return 0.5 * (lo + hi) + 0.5 * (hi - lo) * x, 0.5 * (hi - lo) * w


def norm3(table, n=64):
    """Z = 2 pi int_0^1 L(c) c dc, segment by segment (the integrand is a quadratic there: exact)"""
    M = len(table)
    edges = np.linspace(0.0, 1.0, M)
    c, w = _gl(min(n, 8), edges[:-1], edges[1:])
    return 2.0 * np.pi * float((law(table, c) * c * w).sum())


def norm2(table, n=64):
    """Z_2 = int_{-pi/2}^{pi/2} L(cos phi) cos(phi) d phi, segment by segment in phi (smooth on each)"""
    M = len(table)
    edges = np.arccos(np.linspace(0.0, 1.0, M))  # phi of the nodes, from pi / 2 down to 0
    phi, w = _gl(n, edges[1:], edges[:-1])
    return 2.0 * float((law(table, np.cos(phi)) * np.cos(phi) * w).sum())


def _opening(x, w=W, d=DEPTH):
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    return np.arctan2(-w / 2 - x, d), np.arctan2(w / 2 - x, d)


def source_bottom(table, x, n):
    p1, p2 = _opening(x)
    phi, wphi = _gl(n, p1, p2)  # [x, n]
    psi, wpsi = _gl(n, 0.0, np.pi / 2)  # [n]; the integrand is even in psi
    c = np.cos(phi)[:, :, None] * np.cos(psi)[None, None, :]
    f = law(table, c) * np.cos(phi)[:, :, None] * (np.cos(psi) ** 2)[None, None, :]
    return 2.0 * (f * wphi[:, :, None] * wpsi[None, None, :]).sum((1, 2)) / norm3(table)


def source_bottom_2d(table, x, n):
    p1, p2 = _opening(x)
    phi, wphi = _gl(n, p1, p2)
    return (law(table, np.cos(phi)) * np.cos(phi) * wphi).sum(1) / norm2(table)


def yield_wall(table, z, n, w=W, look_up_at_c=False):
    """z: heights of wall points, < 0.  Either wall: the scene is symmetric.  look_up_at_c: the WRONG integral, Y taken at
    c = cos(phi) cos(psi) — what the test must tell from the right one"""
    z = np.atleast_1d(np.asarray(z, dtype=np.float64))
    phi, wphi = _gl(n, np.zeros_like(z), np.arctan2(w, -z))
    psi, wpsi = _gl(n, 0.0, np.pi / 2)
    mu = (np.cos(phi) if look_up_at_c else np.sin(phi))[:, :, None] * np.cos(psi)[None, None, :]
    f = law(table, mu) * np.sin(phi)[:, :, None] * (np.cos(psi) ** 2)[None, None, :]
    return 2.0 * (f * wphi[:, :, None] * wpsi[None, None, :]).sum((1, 2)) / np.pi


def yield_wall_unit(z, w=W):
    """Y = 1: (1 - cos(phi_max)) / 2"""
    z = np.atleast_1d(np.asarray(z, dtype=np.float64))
    return 0.5 * (1.0 - np.cos(np.arctan2(w, -z)))


def reflectivity_bottom(table, rho, x, n, kmax=80, w=W, d=DEPTH):
    """images |k| > kmax lack at most sum_k rho^|k| (their share of sin(phi)) < rho^kmax: 2e-8 at rho 0.8, kmax 80"""
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    psi, wpsi = _gl(n, 0.0, np.pi / 2)
    cpsi = np.cos(psi)
    out = np.zeros_like(x)
    for k in range(-kmax, kmax + 1):
        a, b = -w / 2 + k * w, w / 2 + k * w
        phi, wphi = _gl(n, np.arctan2(a - x, d), np.arctan2(b - x, d))
        mu = np.abs(np.sin(phi))[:, :, None] * cpsi[None, None, :]
        f = (rho * law(table, mu)) ** abs(k) * np.cos(phi)[:, :, None] * (cpsi ** 2)[None, None, :]
        out += 2.0 * (f * wphi[:, :, None] * wpsi[None, None, :]).sum((1, 2)) / np.pi
    return out


def converged(fn, *args, n):
    """(fn at 2 n nodes, the largest difference to fn at n nodes)"""
    coarse, fine = fn(*args, n), fn(*args, 2 * n)
    return fine, float(np.max(np.abs(fine - coarse)))
