#!/usr/bin/env python3
"""CPU model (numpy, no GPU) of what the generator's sort-bin grid costs the flat-scene trace kernels: the candidates per
packet — the disks whose ball box meets the box around a round's 64 rays — for rays in the order the bins put them.

The scene is C2's: an n x n lattice of disks of pitch 1 (= gridDelta) and radius 0.866 on a plane, the rays' far-plane
crossings uniform over the domain [first centre, last centre].  The key is the generator's own (vr_bin_grid.hpp: one
float fused multiply-add per axis, 8 x 8 tiles, columns in alternating directions); a trace round takes 64 consecutive
rays in bin order (rays of one bin in arbitrary order, as the bin cursors hand the slots out).  A window is a band of
whole tile rows across the full width, so that the walk from tile to tile is the real one.

  --grid plain      ceil(sqrt(rays / rays_per_bin)) equal cells per axis over the extent (VR_BIN_ALIGN=0)
  --grid rule       the aligned grid as bin_grid_aligned (vr_bin_grid.hpp) sizes it
  --grid AxB        cells of A x B lattice cells (axis 1 x axis 2; fractions like 0.5 or 1/3), edges on the lattice lines
  --phase P         ... with the edges moved off the lines by P cells of either axis
  --density R       rays per disk (C2: 100, i.e. 10^8 rays on 1000 x 1000 disks: 100.2 per lattice cell)
  --jitter J        every centre displaced by up to +-J pitch in the plane (not a lattice any more)

Validation (profiles/aligned_bins_ab.txt).  The criterion set for this tool — reproduce the 8.7 candidates per packet of the
committed profile on C2's plain grid — is NOT met: the model gives 8.0 there (and 5.5 on the aligned grid).  The -DVR_DIAG build
of this commit counts "packet prim tests" / "pq done" = 9.52 (plain) and 6.31 (aligned): the model is 16 % and 13 % low — it
leaves out the queries that give up (4.6 % of the attempts, the widest boxes) and the padding of the query box.  What it does
reproduce, nearly, is the RATIO of the two grids: -32 % against the measured -34 %.
"""
import argparse
import math
from fractions import Fraction

import numpy as np

R_DISK = 0.8660254 * (1 + 1e-5)


def rule(ext, rays, per_bin=40, bin_cap=128):
    """bin_grid_aligned (vr_bin_grid.hpp) for a square domain of `ext` lattice cells of pitch 1 that starts on a disk centre
    (origin = lo, so the header's span1 = span2 = ext): (m1, m2, k2) or None where it falls back.  A copy of the header's rule:
    tests/test_bin_grid_host.py holds the two together on seven such parameter sets only — the branches of the 4096-cell cap and a
    domain that does not start on a lattice line are not compared and can drift."""
    rho = rays / (ext * ext)
    mean_hi = 0.5 * bin_cap
    want = min(per_bin, mean_hi)
    span1 = span2 = ext
    m1min = max(1.0, math.ceil(span1 / 4096 - 1e-9))
    m2min = max(1.0, math.ceil(span2 / 4096 - 1e-9))
    m1, m2, k2 = m1min, 1.0, 1.0
    if rho * m1 >= want:
        rho1 = rho * m1
        k2 = max(1.0, math.floor(rho1 / per_bin), math.ceil(rho1 / mean_hi))
        kmax = math.floor(4096 / span2)
        if kmax < 1:
            k2, m2 = 1.0, m2min
        else:
            k2 = min(k2, kmax)
    else:
        A = want / rho
        m2 = max(m2min, math.floor(math.sqrt(A)))
        m1 = max(m1min, math.floor(A / m2 + 0.5))
        if rho * m1 * m2 > mean_hi and m1 > m1min:
            m1 -= 1
    mean = rho * m1 * m2 / k2
    if not (0.5 * want <= mean <= mean_hi):
        return None
    return int(m1), int(m2), int(k2)


def make_grid(args):
    """(T1, T2, scale1, bias1, scale2, bias2, label) of the key: cell = (int)fma(u, scale, bias)"""
    n, ext = args.n, args.n - 1.0
    rays = args.density * n * n
    if args.grid == "plain":
        T = int(min(4096, max(1, math.ceil(math.sqrt(max(rays // args.rays_per_bin, 1))))))
        return T, T, float(T), 0.0, float(T), 0.0, f"plain {T} x {T}, cell {ext / T:.4f}"
    if args.grid == "rule":
        r = rule(ext, rays, args.rays_per_bin, args.bin_cap)
        if r is None:
            raise SystemExit("the rule falls back to the plain grid here")
        c1, c2 = float(r[0]), r[1] / r[2]
    else:
        a, b = args.grid.lower().split("x")
        c1, c2 = float(Fraction(a)), float(Fraction(b))
    # origin at -phase cells (at or below lo = 0 in lattice units measured from the first centre)
    o1, o2 = -(args.phase % 1.0) * c1, -(args.phase % 1.0) * c2
    T1, T2 = math.ceil((ext - o1) / c1 - 1e-6), math.ceil((ext - o2) / c2 - 1e-6)
    return T1, T2, ext / c1, -o1 / c1, ext / c2, -o2 / c2, f"cells {c1:.4g} x {c2:.4g}, phase {args.phase:g}: {T1} x {T2}, {rays / (ext * ext) * c1 * c2:.1f} rays per bin"


def bins_of(x, y, grid, ext):
    T1, T2, s1, b1, s2, b2, _ = grid
    f = np.float32
    u1, u2 = (x.astype(f) * f(1.0 / ext)).astype(f), (y.astype(f) * f(1.0 / ext)).astype(f)
    # (float32 product + sum in float64, rounded once: the fused multiply-add)
    c1 = np.clip((u1.astype(np.float64) * np.float64(f(s1)) + np.float64(f(b1))).astype(f).astype(np.int64), 0, T1 - 1)
    c2 = np.clip((u2.astype(np.float64) * np.float64(f(s2)) + np.float64(f(b2))).astype(f).astype(np.int64), 0, T2 - 1)
    tiles = (T1 + 7) // 8
    row, col = c2 & 7, c1 & 7
    return ((c2 >> 3) * tiles + (c1 >> 3)) * 64 + (col << 3 | np.where(col & 1, 7 - row, row)), c2 >> 3


def window(args, grid, rng, w):
    """candidates of every round of one band of tile rows"""
    n, ext = args.n, args.n - 1.0
    T2, s2, b2 = grid[1], grid[4], grid[5]
    tileRows = (T2 + 7) // 8
    first = int((w + 0.5) / args.windows * max(1, tileRows - args.rows))
    # y range of the band's tile rows (a margin of one cell, trimmed by the tile row below)
    cell2 = ext / s2
    y0 = max(0.0, (first * 8 - b2) * cell2 - cell2)
    y1 = min(ext, ((first + args.rows) * 8 - b2) * cell2 + cell2)
    count = rng.poisson(args.density * args.n * args.n / ext * (y1 - y0))
    x, y = rng.random(count) * ext, y0 + rng.random(count) * (y1 - y0)
    b, trow = bins_of(x, y, grid, ext)
    keep = (trow >= first) & (trow < first + args.rows)
    x, y, b = x[keep], y[keep], b[keep]
    order = np.argsort(b, kind="stable") # (the rays of a bin: generation order, which is random in space)
    x, y = x[order], y[order]
    rounds = len(x) // 64
    x, y = x[: rounds * 64].reshape(rounds, 64), y[: rounds * 64].reshape(rounds, 64)
    xlo, xhi, ylo, yhi = x.min(1) - R_DISK, x.max(1) + R_DISK, y.min(1) - R_DISK, y.max(1) + R_DISK
    if args.jitter == 0.0:
        nx = np.minimum(np.floor(xhi), n - 1) - np.maximum(np.ceil(xlo), 0) + 1
        ny = np.minimum(np.floor(yhi), n - 1) - np.maximum(np.ceil(ylo), 0) + 1
        return nx * ny
    # jittered centres: count them one by one (the band's lattice rows only)
    j0, j1 = max(0, int(math.floor(y0 - 2))), min(n - 1, int(math.ceil(y1 + 2)))
    jr = np.random.default_rng(12345) # (the same cloud for every window and grid)
    dx, dy = (jr.random((n, n)) * 2 - 1) * args.jitter, (jr.random((n, n)) * 2 - 1) * args.jitter
    cand = np.zeros(rounds)
    for r in range(rounds):
        i0, i1 = max(0, int(math.floor(xlo[r] - 1))), min(n - 1, int(math.ceil(xhi[r] + 1)))
        k0, k1 = max(j0, int(math.floor(ylo[r] - 1))), min(j1, int(math.ceil(yhi[r] + 1)))
        I, K = np.meshgrid(np.arange(i0, i1 + 1), np.arange(k0, k1 + 1), indexing="ij")
        cx, cy = I + dx[I, K], K + dy[I, K]
        cand[r] = np.count_nonzero((cx >= xlo[r]) & (cx <= xhi[r]) & (cy >= ylo[r]) & (cy <= yhi[r]))
    return cand


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", default="plain")
    ap.add_argument("--phase", type=float, default=0.0)
    ap.add_argument("--density", type=float, default=100.0)
    ap.add_argument("--jitter", type=float, default=0.0)
    ap.add_argument("--n", type=int, default=1000, help="lattice points per axis")
    ap.add_argument("--rays-per-bin", type=int, default=40)
    ap.add_argument("--bin-cap", type=int, default=128)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--rows", type=int, default=2, help="tile rows per window")
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    grid = make_grid(args)
    rng = np.random.default_rng(args.seed)
    means = []
    for w in range(args.windows):
        c = window(args, grid, rng, w)
        means.append(float(c.mean()))
    print(f"{grid[6]}")
    print("candidates per packet: " + " ".join(f"{m:.2f}" for m in means) + f"  mean {np.mean(means):.2f}")


if __name__ == "__main__":
    main()
