#!/usr/bin/env python3
"""What the angular laws cost (Trace.gatherAngular: gatherPaths weighed by tabulated source radiance, reflectivity and
yield, the gather's own kernel in its PATH 3 instantiation with the laws staged in LDS), on the two scenes of
tools/gather_paths_bench.py — tests/golden/data/trenchGrid3D.dat and the 10^6-disk rippled sheet — at K = 64 and 256
samples per primitive, specular and diffuse, reflectivity 0.7, maxBounces 64.  Per scene, K and reflection, in the same
run and with the same arguments:
  paths      gatherPaths: the PATH 1 kernel, whose text and registers this commit leaves as they were;
  ones       gatherAngular with three all-ones laws (M = 256): the same bits, every look-up made;
  laws       gatherAngular with the laws of the tests: M = 5, R falling from 1 to 0.2, Y rising from 0.5 to 3, L from c^3.
One process, device events on torch's stream around the calls, warm-up rounds first, median over the rounds; `spread` is
(max - min) / median of the gatherPaths rounds, what a ratio has to exceed to mean anything.  Writes
profiles/gather_angular_bench.json (or the path given as the third argument) and prints it as one line.
usage: tools/gather_angular_bench.py [rounds=5] [warmup=2] [out.json]"""
import json
import os
import statistics
import sys

import numpy as np
import torch  # (before the tracing library: one HIP runtime for both)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import viennaray_amd as vr  # noqa: E402
from helpers import trench3d  # noqa: E402

SAMPLES = (64, 256)
KINDS = (vr.GatherReflection.SPECULAR, vr.GatherReflection.DIFFUSE)
RHO, BOUNCES = 0.7, 64
ONES = dict(sourceLaw=np.ones(256, np.float32), reflectivityLaw=np.ones(256, np.float32), yieldLaw=np.ones(256, np.float32))
LAWS = dict(sourceLaw=(np.linspace(0.0, 1.0, 5) ** 3).astype(np.float32), reflectivityLaw=np.linspace(1.0, 0.2, 5).astype(np.float32),
            yieldLaw=np.linspace(0.5, 3.0, 5).astype(np.float32))


def rippled_sheet(n):
    """bench.py's C2_rippled: z = 0.5 sin(x/4) cos(y/4), normals of the height field"""
    pts, _ = vr.io.plane_grid(n, 1.0)
    x, y = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    amp, wave = 0.5, 4.0
    pts = pts.copy()
    pts[:, 2] = (amp * np.sin(x / wave) * np.cos(y / wave)).astype(np.float32)
    nv = np.stack([-amp / wave * np.cos(x / wave) * np.cos(y / wave), amp / wave * np.sin(x / wave) * np.sin(y / wave),
                   np.ones_like(x)], -1)
    return pts.astype(np.float32), (nv / np.linalg.norm(nv, axis=1, keepdims=True)).astype(np.float32)


def scenes():
    gd, pts, nrm = trench3d()
    yield "trenchGrid3D", pts.astype(np.float32), nrm.astype(np.float32), float(gd)
    pts, nrm = rippled_sheet(1000)
    yield "rippled sheet, 10^6 disks", pts, nrm, 1.0


def tracer(pts, nrm, gd):
    t = vr.TraceDisk(3)
    t.setGeometry(pts, nrm, gd)
    t.setBoundaryConditions([vr.BoundaryCondition.PERIODIC_BOUNDARY] * 3)
    t.setParticleType(vr.DiffuseParticle(1.0, "flux"))
    t.setNumberOfRaysFixed(1_000_000)
    t.setUseRandomSeeds(False)
    t.setRngSeed(12345)
    t.applyPrepare()
    return t


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def med(fn, rounds, warmup):
    ms = [timed(fn)[0] for _ in range(warmup + rounds)][warmup:]
    m = statistics.median(ms)
    return dict(median=round(m, 4), min=round(min(ms), 4), spread=round((max(ms) - min(ms)) / m, 4))


def case(name, pts, nrm, gd, rounds, warmup):
    t = tracer(pts, nrm, gd)
    out = dict(scene=name, primitives=int(pts.shape[0]), rounds=rounds, reflectivity=RHO, max_bounces=BOUNCES, samples={})
    for k in SAMPLES:
        r = {}
        for kind in KINDS:
            kw = dict(reflectivity=RHO, reflection=kind, maxBounces=BOUNCES)
            paths = med(lambda: t.gatherPaths(k, **kw), rounds, warmup)
            ones = med(lambda: t.gatherAngular(k, **ONES, **kw), rounds, warmup)
            laws = med(lambda: t.gatherAngular(k, **LAWS, **kw), rounds, warmup)
            same = bool((t.gatherAngular(k, **ONES, **kw) == t.gatherPaths(k, **kw)).all())
            r[kind.name.lower()] = dict(paths_ms=paths, ones_ms=ones, laws_ms=laws, ones_same_bits=same,
                                        ones_over_paths=round(ones["median"] / paths["median"], 4),
                                        laws_over_paths=round(laws["median"] / paths["median"], 4),
                                        mean_flux_laws=round(float(t.gatherAngular(k, **LAWS, **kw).mean()), 5))
        out["samples"][str(k)] = r
    return out


def main():
    args = sys.argv[1:]
    rounds = int(args[0]) if len(args) > 0 else 5
    warmup = int(args[1]) if len(args) > 1 else 2
    path = args[2] if len(args) > 2 else os.path.join(ROOT, "profiles", "gather_angular_bench.json")
    cases = [case(name, p, nr, gd, rounds, warmup) for name, p, nr, gd in scenes()]
    res = dict(tool="gather_angular_bench", device=torch.cuda.get_device_name(0), cases=cases)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
