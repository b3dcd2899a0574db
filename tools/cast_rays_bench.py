#!/usr/bin/env python3
"""What a closest-hit query for the caller's rays costs (Trace.castRays), on C2's plane of 10^6 disks and on
tests/golden/data/trenchGrid3D.dat, for two kinds of rays:

  coherent    a regular pencil from above the scene, row by row: neighbouring rays walk alike as they are;
  scattered   rays leaving random surface points (a primitive's centre, lifted off it by 1e-3 gridDelta) in cosine
              directions about the primitive's normal, in random order.

Each kind is cast from device tensors with the ray sort forced on (VR_CAST_SORT_MIN=0) and off, the variants interleaved
round by round in one process, at a ladder of ray counts up to `rays`; timed with device events on torch's stream around
the call (the hand-over makes that stream wait for the library's), warm-up rounds first, median and minimum over the
rounds.  `crossover` is the smallest count of the ladder from which the sorted cast of the scattered kind is the faster
one on every larger count too, per scene and over both (null: never).  The same rays also go through debugIntersect
(vr_debug_intersect: host arrays, one segment, no walls followed), the only way to these answers before castRays, by
the wall clock; `cast_one_segment` is castRays with followBoundaries off on the same device tensors, for that comparison.
Prints one JSON line.
usage: tools/cast_rays_bench.py [rays=10000000] [rounds=7] [warmup=2]"""
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

NEVER = "4294967295"
LADDER = (1 << 12, 1 << 14, 1 << 16, 1 << 17, 1 << 18, 1 << 19, 1 << 20, 1 << 22)


def scenes():
    pts, nrm = vr.io.plane_grid(1000, 1.0)
    yield "C2 plane, 10^6 disks", pts.astype(np.float32), nrm.astype(np.float32), 1.0
    gd, pts, nrm = trench3d()
    yield "trenchGrid3D", pts.astype(np.float32), nrm.astype(np.float32), float(gd)


def coherent_rays(pts, gd, m):
    """a regular pencil over the scene's plan, one gridDelta above its top, slightly off the vertical"""
    lo, hi = pts.min(0), pts.max(0)
    nx = int(np.ceil(np.sqrt(m)))
    ix, iy = np.divmod(np.arange(m), nx)
    o = np.empty((m, 3), np.float32)
    o[:, 0] = lo[0] + (hi[0] - lo[0]) * (ix + 0.5) / nx
    o[:, 1] = lo[1] + (hi[1] - lo[1]) * (iy + 0.5) / nx
    o[:, 2] = hi[2] + gd
    d = np.tile(np.array([[0.05, 0.02, -1.0]], np.float32), (m, 1))
    return o, d


def scattered_rays(pts, nrm, gd, m, rng):
    """cosine-distributed directions about the normals of random primitives, from just off their centres"""
    j = rng.integers(0, pts.shape[0], m)
    n = nrm[j].astype(np.float64)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    helper = np.where(np.abs(n[:, [0]]) < 0.9, np.array([[1.0, 0, 0]]), np.array([[0, 1.0, 0]]))
    u = np.cross(n, helper)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = np.cross(n, u)
    r1, r2 = rng.uniform(size=m), rng.uniform(size=m)
    s, phi = np.sqrt(r1), 2 * np.pi * r2
    d = (s * np.cos(phi))[:, None] * u + (s * np.sin(phi))[:, None] * v + np.sqrt(1 - r1)[:, None] * n
    o = pts[j].astype(np.float64) + 1e-3 * gd * n
    return o.astype(np.float32), d.astype(np.float32)


def stat(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4))


def timed_cast(t, o, d, **kw):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = t.castRays(o, d, **kw)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def crossover_of(rows):
    """rows: [(m, sort median, nosort median)] ascending in m -> the smallest m from which sort wins at every larger m too"""
    best = None
    for m, s, n in reversed(rows):
        if s < n:
            best = m
        else:
            break
    return best


def case(name, pts, nrm, gd, rays, rounds, warmup):
    t = vr.TraceDisk(3)
    t.setGeometry(pts, nrm, gd)
    t.setBoundaryConditions([vr.BoundaryCondition.REFLECTIVE_BOUNDARY] * 3)
    t.setParticleType(vr.DiffuseParticle(1.0, "flux"))
    t.setNumberOfRaysFixed(1_000_000)
    t.setUseRandomSeeds(False)
    t.setRngSeed(12345)
    t.applyPrepare()
    rng = np.random.default_rng(1)
    host = {"coherent": coherent_rays(pts, gd, rays), "scattered": scattered_rays(pts, nrm, gd, rays, rng)}
    dev = {k: (torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()) for k, (o, d) in host.items()}
    ladder = sorted({m for m in LADDER if m < rays} | {rays})
    out = dict(scene=name, primitives=int(pts.shape[0]), rays=int(rays), rounds=rounds, kinds={})
    for kind, (o, d) in dev.items():
        sizes = []
        for m in ladder:
            # (a prefix of the scattered rays is scattered; of the pencil, its first rows: a strip of the scene)
            om, dm = o[:m], d[:m]
            times = {"sort": [], "nosort": []}
            for k in range(warmup + rounds):
                for s, row in times.items():
                    os.environ["VR_CAST_SORT_MIN"] = "0" if s == "sort" else NEVER
                    ms, res = timed_cast(t, om, dm)
                    if k >= warmup:
                        row.append(ms)
            prim = res[0]
            sizes.append(dict(rays=int(m), sort_ms=stat(times["sort"]), nosort_ms=stat(times["nosort"]),
                              sort_rays_per_s=round(m / (statistics.median(times["sort"]) * 1e-3)),
                              nosort_rays_per_s=round(m / (statistics.median(times["nosort"]) * 1e-3)),
                              hit_share=round(float((prim >= 0).float().mean()), 4)))
        os.environ["VR_CAST_SORT_MIN"] = NEVER
        one = [timed_cast(t, o, d, followBoundaries=False)[0] for _ in range(warmup + min(rounds, 3))][warmup:]
        del os.environ["VR_CAST_SORT_MIN"]
        ho, hd = host[kind]
        dbg = []
        for _ in range(1 + min(rounds, 3)):
            t0 = time.perf_counter()
            g, p, tt = t.debugIntersect(ho, hd)
            dbg.append((time.perf_counter() - t0) * 1e3)
        dbg = dbg[1:]
        # the same answers: debugIntersect's geometry hits are the one-segment cast's primitives
        prim1 = t.castRays(o, d, followBoundaries=False)[0].cpu().numpy()
        same = bool(np.array_equal(prim1 >= 0, g == 1) and np.array_equal(prim1[g == 1], p[g == 1].astype(np.int32)))
        out["kinds"][kind] = dict(
            sizes=sizes, crossover=crossover_of([(s["rays"], s["sort_ms"]["median"], s["nosort_ms"]["median"]) for s in sizes]),
            cast_one_segment_nosort_ms=stat(one), debug_intersect_ms=stat(dbg),
            debug_intersect_rays_per_s=round(rays / (statistics.median(dbg) * 1e-3)),
            debug_intersect_over_cast_one_segment=round(statistics.median(dbg) / statistics.median(one), 1),
            same_answers_as_debug_intersect=same)
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rays = int(args[0]) if len(args) > 0 else 10_000_000
    rounds = int(args[1]) if len(args) > 1 else 7
    warmup = int(args[2]) if len(args) > 2 else 2
    cases = [case(name, p, n, gd, rays, rounds, warmup) for name, p, n, gd in scenes()]
    per_scene = [c["kinds"]["scattered"]["crossover"] for c in cases]
    both = None if any(x is None for x in per_scene) else max(per_scene)
    print(json.dumps(dict(tool="cast_rays_bench", device=torch.cuda.get_device_name(0), cases=cases,
                          scattered_crossover_per_scene=per_scene, scattered_crossover_both_scenes=both)), flush=True)


if __name__ == "__main__":
    main()
