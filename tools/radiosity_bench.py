#!/usr/bin/env python3
"""What solveRadiosity costs (Trace.solveRadiosity: gatherFlux's samples walked once into a link table, then one pass over
the table per iteration), on tests/golden/data/trenchGrid3D.dat and on the 10^6-disk rippled sheet (bench.py's
C2_rippled), at K = 64 and 256 samples per primitive.  Per scene and K:
  1. the link build against gatherFlux(K), the same call without recording;
  2. one iteration against one gatherFlux(K, emission=...): 64 iteration kernels launched back to back between two
     device events (vr_debug_radiosity_time_iterations, reflectivity 0.99), per kernel;
  3. the iteration's link bytes per second (4 x slots x K per iteration), and the same kernel with non-temporal loads
     for the stream beside the plain ones a solve uses;
  4. a whole solve at sticking 0.1 and 0.01 (tolerance 1e-4), with its iteration count, against that many times one
     gatherFlux with emission;
  5. for orientation only: the relative L2 difference to a forward DiffuseParticle(s) apply of 10^8 rays, SOURCE-normalised.
One process, device events on torch's stream around the calls, warm-up rounds first, median over the rounds.  Writes
profiles/radiosity_bench.json and prints it as one line.
usage: tools/radiosity_bench.py [rounds=5] [warmup=2] [forward_rays=100000000]"""
import ctypes as C
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


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def med(fn, rounds, warmup):
    ms = [timed(fn)[0] for _ in range(warmup + rounds)][warmup:]
    return dict(median=round(statistics.median(ms), 4), min=round(min(ms), 4))


def iteration_ms(t, rho, nontemporal, rounds, warmup, count=64):
    """ms per iteration kernel over the resident table: `count` launches back to back between two device events
    (vr_debug_radiosity_time_iterations: every launch runs, converged or not), median over the rounds"""
    ms = []
    for _ in range(warmup + rounds):
        one = C.c_float(0.0)
        t._check(t._L.vr_debug_radiosity_time_iterations(t._h, rho, count, int(nontemporal), C.byref(one)))
        ms.append(one.value)
    return statistics.median(ms[warmup:])


def case(name, pts, nrm, gd, rounds, warmup, forward_rays):
    t = vr.TraceDisk(3)
    t.setGeometry(pts, nrm, gd)
    t.setBoundaryConditions([vr.BoundaryCondition.PERIODIC_BOUNDARY] * 3)
    t.setParticleType(vr.DiffuseParticle(1.0, "flux"))
    t.setNumberOfRaysFixed(1_000_000)
    t.setUseRandomSeeds(False)
    t.setRngSeed(12345)
    t.applyPrepare()
    n = int(pts.shape[0])
    slots = (n + 63) // 64 * 64
    out = dict(scene=name, primitives=n, rounds=rounds, samples={})
    solved = {}
    for k in (64, 256):
        r = dict(link_bytes=t.radiosityLinkBytes(k))
        r["gather_ms"] = med(lambda: t.gatherFlux(k), rounds, warmup)
        r["link_build_ms"] = med(lambda: t.radiosityLinks(k), rounds, warmup)
        em = t.gatherFlux(k) * 0.9
        r["gather_with_emission_ms"] = med(lambda: t.gatherFlux(k, emission=em), rounds, warmup)
        it = iteration_ms(t, 0.99, False, rounds, warmup)  # plain loads for the link stream: what a solve launches
        r["iteration_ms"] = round(it, 5)
        r["iteration_link_gbytes_per_s"] = round(4.0 * slots * k / (it * 1e-3) / 1e9, 1)
        r["iteration_share_of_8_tbytes_per_s"] = round(4.0 * slots * k / (it * 1e-3) / 8e12, 4)
        r["iteration_mlinks_per_s"] = round(n * k / (it * 1e-3) / 1e6, 1)
        r["iteration_nontemporal_loads_ms"] = round(iteration_ms(t, 0.99, True, rounds, warmup), 5)
        for s in (0.1, 0.01):
            flux, its, res = t.solveRadiosity(k, sticking=torch.full((n,), s, dtype=torch.float32, device="cuda"), returnInfo=True)
            ms = med(lambda: t.solveRadiosity(k, sticking=torch.full((n,), s, dtype=torch.float32, device="cuda")), rounds, warmup)
            r["solve_s%g" % s] = dict(ms=ms, iterations=its, residual=res, mean_flux=round(float(flux.mean()), 5),
                                      chained_gathers_ms=round(its * r["gather_with_emission_ms"]["median"], 3))
            solved[(k, s)] = flux.cpu().numpy().astype(np.float64)
        out["samples"][str(k)] = r
    t.freeRadiosityLinks()
    # 5. a forward apply, for orientation only
    out["forward"] = {}
    for s in (0.1, 0.01):
        t.setParticleType(vr.DiffuseParticle(s, "flux"))
        t.setNumberOfRaysFixed(forward_rays)
        t.apply()  # (the first apply of a ray count sizes the ray stream: not timed)
        ms, _ = timed(t.apply)
        fwd = t.getFluxNormalized().astype(np.float64)
        out["forward"]["s%g" % s] = dict(rays=forward_rays, apply_ms=round(ms, 2), mean_flux=round(float(fwd.mean()), 5), **{
            "rel_l2_to_solve_K%d" % k: round(float(np.linalg.norm(solved[(k, s)] - fwd) / np.linalg.norm(fwd)), 5) for k in (64, 256)})
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rounds = int(args[0]) if len(args) > 0 else 5
    warmup = int(args[1]) if len(args) > 1 else 2
    forward_rays = int(args[2]) if len(args) > 2 else 100_000_000
    cases = [case(name, p, nr, gd, rounds, warmup, forward_rays) for name, p, nr, gd in scenes()]
    res = dict(tool="radiosity_bench", device=torch.cuda.get_device_name(0), cases=cases)
    with open(os.path.join(ROOT, "profiles", "radiosity_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
