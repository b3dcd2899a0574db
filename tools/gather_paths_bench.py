#!/usr/bin/env python3
"""What gatherPaths costs (Trace.gatherPaths: gatherFlux's samples followed back through their reflections in the
gather's own kernel), on tests/golden/data/trenchGrid3D.dat and on the 10^6-disk rippled sheet (bench.py's C2_rippled), at
K = 64 and 256 samples per primitive, specular and diffuse, reflectivity 0.7 and 0.99, maxBounces 64.  Per scene and K:
  1. gatherFlux(K), and gatherPaths(K, maxBounces=0): the same walk in the path instantiation;
  2. every gatherPaths call;
  3. segments per path and the useful-lane share of the segment loop, from the counters of a -DVR_DIAG build of the
     library (make -C viennaray_amd/csrc diag) run once per setting in a child process: a round of segments occupies
     the wave until the longest path of its 64 has finished the segment; null where that build is absent;
  4. for orientation only (trench): a forward SpecularParticle(0.3) apply of 10^8 rays, with the relative L2 difference
     of its SOURCE-normalised flux to gatherPaths(K, sticking=0.3, SPECULAR).
One process for the timings, device events on torch's stream around the calls, warm-up rounds first, median over the
rounds.  Writes profiles/gather_paths_bench.json and prints it as one line.
usage: tools/gather_paths_bench.py [rounds=5] [warmup=2] [forward_rays=100000000]"""
import json
import os
import re
import statistics
import subprocess
import sys

import numpy as np
import torch  # (before the tracing library: one HIP runtime for both)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import viennaray_amd as vr  # noqa: E402
from helpers import trench3d  # noqa: E402

DIAG_LIB = os.path.join(ROOT, "viennaray_amd", "libviennaray_amd_diag.so")
SAMPLES = (64, 256)
SETTINGS = [(kind, rho) for kind in (vr.GatherReflection.SPECULAR, vr.GatherReflection.DIFFUSE) for rho in (0.7, 0.99)]
BOUNCES = 64


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
    return dict(median=round(statistics.median(ms), 4), min=round(min(ms), 4))


def key(kind, rho):
    return "%s_rho%g" % (kind.name.lower(), rho)


def diag_child():
    """under the -DVR_DIAG library: every setting once; the library prints one line of counters per call on stderr"""
    for name, pts, nrm, gd in scenes():
        t = tracer(pts, nrm, gd)
        for k in SAMPLES:
            for kind, rho in SETTINGS:
                sys.stderr.write("diag case %s | %d | %s\n" % (name, k, key(kind, rho)))
                sys.stderr.flush()
                t.gatherPaths(k, reflectivity=rho, reflection=kind, maxBounces=BOUNCES)
                torch.cuda.synchronize()


def lane_counters():
    """{(scene, K, setting): (rounds, segments, paths)} from a child process under the diag library, or {} without it"""
    if not os.path.exists(DIAG_LIB):
        return {}
    env = dict(os.environ, VR_LIB_PATH=DIAG_LIB)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--diag-child"], env=env, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-2000:])
        return {}
    out, case = {}, None
    for line in p.stderr.splitlines():
        m = re.match(r"diag case (.*) \| (\d+) \| (\S+)$", line)
        if m:
            case = (m.group(1), int(m.group(2)), m.group(3))
        m = re.match(r"diag gather paths: rounds (\d+) segments (\d+) paths (\d+)$", line)
        if m and case:
            out[case] = tuple(int(v) for v in m.groups())
    return out


def case(name, pts, nrm, gd, rounds, warmup, forward_rays, lanes):
    t = tracer(pts, nrm, gd)
    n = int(pts.shape[0])
    out = dict(scene=name, primitives=n, rounds=rounds, max_bounces=BOUNCES, samples={})
    specular = {}
    for k in SAMPLES:
        r = dict(gather_flux_ms=med(lambda: t.gatherFlux(k), rounds, warmup),
                 paths_no_bounce_ms=med(lambda: t.gatherPaths(k, reflectivity=0.7, maxBounces=0), rounds, warmup))
        for kind, rho in SETTINGS:
            ms = med(lambda: t.gatherPaths(k, reflectivity=rho, reflection=kind, maxBounces=BOUNCES), rounds, warmup)
            flux = t.gatherPaths(k, reflectivity=rho, reflection=kind, maxBounces=BOUNCES)
            e = dict(ms=ms, mean_flux=round(float(flux.mean()), 5), mpaths_per_s=round(n * k / (ms["median"] * 1e-3) / 1e6, 1))
            c = lanes.get((name, k, key(kind, rho)))
            e["segments_per_path"] = round(c[1] / c[2], 3) if c else None
            e["useful_lane_share"] = round(c[1] / (64.0 * c[0]), 4) if c else None
            e["msegments_per_s"] = round(c[1] / (ms["median"] * 1e-3) / 1e6, 1) if c else None
            r[key(kind, rho)] = e
        if forward_rays:
            specular[k] = t.gatherPaths(k, sticking=0.3, reflection=vr.GatherReflection.SPECULAR, maxBounces=BOUNCES).cpu().numpy().astype(np.float64)
        out["samples"][str(k)] = r
    if forward_rays:  # for orientation only
        t.setParticleType(vr.SpecularParticle(0.3, 1.0, "flux"))
        t.setNumberOfRaysFixed(forward_rays)
        t.apply()  # (the first apply of a ray count sizes the ray stream: not timed)
        ms, _ = timed(t.apply)
        fwd = t.getFluxNormalized().astype(np.float64)
        out["forward_specular_s0.3"] = dict(rays=forward_rays, apply_ms=round(ms, 2), mean_flux=round(float(fwd.mean()), 5), **{
            "rel_l2_to_paths_K%d" % k: round(float(np.linalg.norm(specular[k] - fwd) / np.linalg.norm(fwd)), 5) for k in SAMPLES})
    return out


def main():
    if "--diag-child" in sys.argv:
        return diag_child()
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rounds = int(args[0]) if len(args) > 0 else 5
    warmup = int(args[1]) if len(args) > 1 else 2
    forward_rays = int(args[2]) if len(args) > 2 else 100_000_000
    lanes = lane_counters()
    cases = [case(name, p, nr, gd, rounds, warmup, forward_rays if name == "trenchGrid3D" else 0, lanes)
             for name, p, nr, gd in scenes()]
    res = dict(tool="gather_paths_bench", device=torch.cuda.get_device_name(0), lane_counters=bool(lanes), cases=cases)
    with open(os.path.join(ROOT, "profiles", "gather_paths_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
