#!/usr/bin/env python3
"""What the host round trip of a time step costs: a surface that moves every step, traced

  the host way     setGeometry(numpy points) + apply + getFluxNormalized        (H2D rows, host passes, D2H flux)
  the device way   setGeometry(torch tensors) + apply + getFluxTensor           (everything stays in HBM)

in ONE process with one library, the two ways alternating step by step, on C2's plane rippled by half a grid cell
(10^6 disks) and on trenchGrid3D.dat, at 10^6 and 10^7 rays.  A step is timed as a whole (wall clock, the device way
including a final torch.cuda.synchronize()) and per stage: set, prepare, launch (+ finish), result.  The points of a
step are ready before its clock starts (a ring of surfaces, each a little different: the producer is not what is
measured); apply() does not collect getLocalData() on either way.  Prints one JSON line.

--triangles: what handing over a triangle mesh costs — a rippled grid mesh of about 10^6 triangles, set-geometry +
vr_apply_prepare timed for setGeometry(numpy arrays) and for setGeometry(torch tensors), alternating step by step in
one process (a ring of meshes as above; the device way's clock includes a final torch.cuda.synchronize()).
usage: tools/device_geometry_bench.py [--triangles] [steps=20] [warmup=3]"""
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
import viennaray_amd as vr  # noqa: E402
from helpers import trench3d  # noqa: E402

RING = 4
SOURCE = vr.NormalizationType.SOURCE


def rippled_plane(n, phase):
    """bench.py's C2_rippled (z = 0.5 sin(x/4) cos(y/4), normals of the height field), shifted by `phase`"""
    pts, _ = vr.io.plane_grid(n, 1.0)
    x, y = pts[:, 0].astype(np.float64) + phase, pts[:, 1].astype(np.float64)
    amp, wave = 0.5, 4.0
    pts[:, 2] = (amp * np.sin(x / wave) * np.cos(y / wave)).astype(np.float32)
    nv = np.stack([-amp / wave * np.cos(x / wave) * np.cos(y / wave), amp / wave * np.sin(x / wave) * np.sin(y / wave),
                   np.ones_like(x)], -1)
    return 1.0, pts, (nv / np.linalg.norm(nv, axis=1, keepdims=True)).astype(np.float32)


def surfaces(name):
    if name == "C2_rippled":
        return [rippled_plane(1000, 0.37 * k) for k in range(RING)], 1.0
    gd, p, n = trench3d()
    out = []
    for k in range(RING):  # the trench, moved a little along its normals
        out.append((gd, (p + np.float32(0.01 * k * gd) * n).astype(np.float32), n))
    return out, 0.1


def tracer(sticking, rays):
    t = vr.TraceDisk(3)
    t.setBoundaryConditions([vr.BoundaryCondition.PERIODIC_BOUNDARY] * 3)
    t.setParticleType(vr.DiffuseParticle(sticking, "flux"))
    t.setNumberOfRaysFixed(rays)
    t.setUseRandomSeeds(False)
    t.setRngSeed(12345)
    return t


def step(t, gd, p, n, on_device):
    c = [time.perf_counter()]
    t.setGeometry(p, n, gd)
    c.append(time.perf_counter())
    t.applyPrepare()
    c.append(time.perf_counter())
    t.applyLaunch()
    t.applyFinish(collect=False)
    c.append(time.perf_counter())
    if on_device:
        f = t.getFluxTensor(0, SOURCE)
        torch.cuda.synchronize()
    else:
        f = t.getFluxNormalized(SOURCE)
    c.append(time.perf_counter())
    ms = [(b - a) * 1e3 for a, b in zip(c, c[1:])]
    return dict(set=ms[0], prepare=ms[1], launch=ms[2], result=ms[3], step=(c[-1] - c[0]) * 1e3), f


def case(name, rays, steps, warmup):
    surf, sticking = surfaces(name)
    dev = [(gd, torch.from_numpy(p).cuda(), torch.from_numpy(n).cuda()) for gd, p, n in surf]
    torch.cuda.synchronize()
    th, td = tracer(sticking, rays), tracer(sticking, rays)
    rows = {"host": [], "device": []}
    same = True
    for k in range(warmup + steps):
        th.setRunNumber(1)
        td.setRunNumber(1)
        gd, p, n = surf[k % RING]
        a, fh = step(th, gd, p, n, False)
        b, fd = step(td, *dev[k % RING], True)
        same = same and bool(np.array_equal(fh, fd.cpu().numpy()))
        if k >= warmup:
            rows["host"].append(a)
            rows["device"].append(b)
    med = {w: {s: round(statistics.median(r[s] for r in rows[w]), 4) for s in ("step", "set", "prepare", "launch", "result")}
           for w in rows}
    return dict(scene=name, disks=int(surf[0][1].shape[0]), rays=rays, sticking=sticking, steps=steps, median_ms=med,
                device_not_slower=med["device"]["step"] <= med["host"]["step"], flux_bit_equal=same, trace_mode=td.traceMode())


def grid_mesh(n, phase):
    """(n + 1)^2 vertices on the unit grid, z as rippled_plane's, two triangles per cell: 2 n^2 triangles"""
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    x, y = j.ravel().astype(np.float64), i.ravel().astype(np.float64)
    v = np.stack([x, y, 0.5 * np.sin((x + phase) / 4.0) * np.cos(y / 4.0)], axis=1).astype(np.float32)
    a = (i[:-1, :-1] * (n + 1) + j[:-1, :-1]).ravel()
    b, d, e = a + 1, a + n + 1, a + n + 2
    t = np.empty((2 * a.size, 3), dtype=np.uint32)
    t[0::2] = np.stack([a, b, d], 1)
    t[1::2] = np.stack([b, e, d], 1)
    return v, t


def triangle_case(rays, steps, warmup, n=707):
    ring = [grid_mesh(n, 0.37 * k) for k in range(RING)]
    dev = [(torch.from_numpy(v).cuda(), torch.from_numpy(t.view(np.int32)).cuda()) for v, t in ring]
    torch.cuda.synchronize()
    tracers = []
    for _ in range(2):
        t = vr.TraceTriangle(3)
        t.setBoundaryConditions([vr.BoundaryCondition.PERIODIC_BOUNDARY] * 3)
        t.setParticleType(vr.DiffuseParticle(1.0, "flux"))
        t.setNumberOfRaysFixed(rays)
        t.setUseRandomSeeds(False)
        t.setRngSeed(12345)
        tracers.append(t)
    th, td = tracers
    rows = {"host": [], "device": []}

    def timed(t, v, tri, on_device):
        c = [time.perf_counter()]
        t.setGeometry(v, tri, 1.0)
        c.append(time.perf_counter())
        t.applyPrepare()
        if on_device:
            torch.cuda.synchronize()
        c.append(time.perf_counter())
        return dict(set=(c[1] - c[0]) * 1e3, prepare=(c[2] - c[1]) * 1e3, both=(c[2] - c[0]) * 1e3)

    for k in range(warmup + steps):
        a = timed(th, *ring[k % RING], False)
        b = timed(td, *dev[k % RING], True)
        if k >= warmup:
            rows["host"].append(a)
            rows["device"].append(b)
    for t in tracers:  # one trace each on the last mesh: the two ways give the same flux
        t.applyLaunch()
        t.applyFinish(collect=False)
    same = bool(np.array_equal(th.getFluxNormalized(SOURCE), td.getFluxNormalized(SOURCE)))
    stat = {w: {s: dict(median=round(statistics.median(r[s] for r in rows[w]), 4), min=round(min(r[s] for r in rows[w]), 4),
                        max=round(max(r[s] for r in rows[w]), 4)) for s in ("both", "set", "prepare")} for w in rows}
    return dict(scene="grid_mesh", triangles=int(ring[0][1].shape[0]), vertices=int(ring[0][0].shape[0]), rays=rays,
                steps=steps, ms=stat, device_not_slower=stat["device"]["both"]["median"] <= stat["host"]["both"]["median"],
                flux_bit_equal=same)


def main():
    args = [a for a in sys.argv[1:] if a != "--triangles"]
    steps = int(args[0]) if len(args) > 0 else 20
    warmup = int(args[1]) if len(args) > 1 else 3
    if "--triangles" in sys.argv[1:]:
        print(json.dumps(dict(tool="device_geometry_bench", mode="triangles", device=torch.cuda.get_device_name(0),
                              cases=[triangle_case(1_000_000, steps, warmup)])), flush=True)
        return
    cases = [case(name, rays, steps, warmup) for name in ("C2_rippled", "trench3d") for rays in (1_000_000, 10_000_000)]
    print(json.dumps(dict(tool="device_geometry_bench", device=torch.cuda.get_device_name(0), cases=cases)), flush=True)


if __name__ == "__main__":
    main()
