#!/usr/bin/env python3
"""What mapping per-primitive values to a caller's points costs (Trace.mapToPoints / getFluxAtPoints), on 10^6 query
points over C2's plane of 10^6 disks and over trenchMesh.dat subdivided three times (819 200 triangles):

  the device call   getFluxAtPoints(points tensor, radius = 2 gridDelta): flux, walk and result stay in HBM; timed with
                    the query sort forced on (VR_MAP_SORT_MIN=0) and off, on the queries in primitive order ("ordered":
                    the centres, jittered by 0.4 gridDelta) and on a random permutation of them ("shuffled"), the four
                    variants interleaved round by round in one process;
  the host path     what a caller had before: getFluxTensor -> .cpu() (download), scipy.spatial.cKDTree over the centres
                    (built per step: the surface moves), the same weighted mean from its k = 32 nearest within the radius
                    (nearest centre where nothing is in range), upload of the result.  None of it is code of this feature:
                    the parent commit runs it as it is.  Without scipy only the two transfers are timed, and the tool says so.

Wall clock around a torch.cuda.synchronize(); median and minimum over the rounds.  With a VR_DIAG build of the library
(VR_LIB_PATH=viennaray_amd/libviennaray_amd_diag.so) and --visits the library reports the node visits per query of every
call on stderr.  Prints one JSON line.
usage: tools/map_points_bench.py [--visits] [rounds=7] [warmup=2] [queries=1000000]"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch  # (before the tracing library: one HIP runtime for both)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
if "--visits" in sys.argv[1:]:
    os.environ["VR_PRINT_LAUNCHES"] = "1"  # (read at prepare; a VR_DIAG build prints the map's node visits)
import viennaray_amd as vr  # noqa: E402
from helpers import trench_mesh  # noqa: E402

try:
    from scipy.spatial import cKDTree
except Exception:  # noqa: BLE001
    cKDTree = None

NEVER = "4294967295"
WORKERS = min(16, os.cpu_count() or 1)  # threads of the k-d tree queries


def subdivided(v, t, levels):
    """every triangle split into four at its edge midpoints, `levels` times (vertices not shared)"""
    tri = v[t.astype(np.int64)].astype(np.float64)  # [nt, 3, 3]
    for _ in range(levels):
        a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
        ab, bc, ca = 0.5 * (a + b), 0.5 * (b + c), 0.5 * (c + a)
        tri = np.concatenate([np.stack(x, 1) for x in ((a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca))])
    verts = tri.reshape(-1, 3).astype(np.float32)
    return verts, np.arange(verts.shape[0], dtype=np.uint32).reshape(-1, 3)


def scenes():
    pts, nrm = vr.io.plane_grid(1000, 1.0)
    t = vr.TraceDisk(3)
    t.setGeometry(pts, nrm, 1.0)
    yield "C2 disks", t, 3, 1.0, pts
    gd, v, tri = trench_mesh()
    v, tri = subdivided(v, tri, 3)
    t = vr.TraceTriangle(3)
    t.setGeometry(v, tri, gd / 8)
    c = ((v[tri[:, 0]] + v[tri[:, 1]]) + v[tri[:, 2]]) * np.float32(1.0 / 3.0)
    yield "trenchMesh x 64", t, 3, gd / 8, c


def host_path(flux_tensor, centres, pts, radius):
    """download, k-d tree, weighted mean, upload: the stages' milliseconds"""
    c = [time.perf_counter()]
    f = flux_tensor.cpu().numpy()
    c.append(time.perf_counter())
    if cKDTree is not None:
        tree = cKDTree(centres)
        c.append(time.perf_counter())
        d, j = tree.query(pts, k=32, distance_upper_bound=radius, workers=WORKERS)
        w = np.where(np.isfinite(d), 1.0 - d / radius, 0.0)
        fj = f[np.minimum(j, f.size - 1)]
        sw = w.sum(1)
        with np.errstate(invalid="ignore", divide="ignore"):
            out = (w * fj).sum(1) / sw
        none = ~(sw > 0)
        if none.any():
            out[none] = f[tree.query(pts[none], k=1, workers=WORKERS)[1]]
        out = out.astype(np.float32)
    else:
        c.append(time.perf_counter())
        out = np.zeros(pts.shape[0], np.float32)
    c.append(time.perf_counter())
    up = torch.from_numpy(out).cuda()
    torch.cuda.synchronize()
    c.append(time.perf_counter())
    ms = [(b - a) * 1e3 for a, b in zip(c, c[1:])]
    return dict(download=ms[0], tree_build=ms[1], query=ms[2], upload=ms[3], total=(c[-1] - c[0]) * 1e3), up


def stat(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4))


def case(name, t, D, gd, centres, rounds, warmup, m):
    t.setBoundaryConditions([vr.BoundaryCondition.PERIODIC_BOUNDARY] * D)
    t.setParticleType(vr.DiffuseParticle(1.0, "flux"))
    t.setNumberOfRaysFixed(2_000_000)
    t.setUseRandomSeeds(False)
    t.setRngSeed(12345)
    t.apply(collect=False)
    rng = np.random.default_rng(1)
    n = centres.shape[0]
    own = np.arange(m) % n
    ordered = (centres[own] + rng.uniform(-0.4, 0.4, (m, 3)).astype(np.float32) * np.float32(gd)).astype(np.float32)
    shuffled = np.ascontiguousarray(ordered[rng.permutation(m)])
    radius = 2.0 * gd
    dev = {"ordered": torch.from_numpy(ordered).cuda(), "shuffled": torch.from_numpy(shuffled).cuda()}
    times = {(o, s): [] for o in dev for s in ("sort", "nosort")}
    for k in range(warmup + rounds):
        for (o, s), row in times.items():
            os.environ["VR_MAP_SORT_MIN"] = "0" if s == "sort" else NEVER
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = t.getFluxAtPoints(dev[o], radius=radius)
            torch.cuda.synchronize()
            if k >= warmup:
                row.append((time.perf_counter() - t0) * 1e3)
    del os.environ["VR_MAP_SORT_MIN"]
    host_rows = []
    agree = None
    for k in range(min(rounds, 3)):
        row, up = host_path(t.getFluxTensor(0), centres, shuffled, radius)
        host_rows.append(row)
        if cKDTree is not None:
            got = t.getFluxAtPoints(dev["shuffled"], radius=radius)
            agree = float((got - up).abs().max())
    host = {s: stat([r[s] for r in host_rows]) for s in host_rows[0]}
    device = {f"{o}/{s}": stat(v) for (o, s), v in times.items()}
    best = min(device[f"shuffled/{s}"]["median"] for s in ("sort", "nosort"))
    return dict(scene=name, primitives=int(n), queries=int(m), radius=radius, rounds=rounds, device_ms=device, host_ms=host,
                host_query="scipy.spatial.cKDTree" if cKDTree is not None else "scipy is not available: transfers only",
                host_over_device_shuffled=round(host["total"]["median"] / best, 2), max_abs_difference_to_host=agree)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rounds = int(args[0]) if len(args) > 0 else 7
    warmup = int(args[1]) if len(args) > 1 else 2
    m = int(args[2]) if len(args) > 2 else 1_000_000
    cases = [case(name, t, D, gd, c, rounds, warmup, m) for name, t, D, gd, c in scenes()]
    print(json.dumps(dict(tool="map_points_bench", device=torch.cuda.get_device_name(0), cases=cases)), flush=True)


if __name__ == "__main__":
    main()
