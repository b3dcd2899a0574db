#!/usr/bin/env python3
"""Surface source: one apply() with the device generator against the same rays through the host-ray path
(vr_set_host_rays + vr_set_host_ray_weights) of a baseline library — VR_BASELINE_LIB, e.g. a build of an earlier commit
made with tools/build_variant.sh; default: this build.  Every measurement is a child process (warm-up apply, then one
timed apply); the two alternate, `rounds` times.  A numpy sampler of a tenth of the rays is timed once, separately.
usage: tools/surface_source_bench.py <trench3d|trench2d> <raysPerPoint> [rounds]        (driver)
       tools/surface_source_bench.py child <variant> <scene> <R> <rayfile>             (one measurement)"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OFFSET, AREA, SEED, STICKING = 1e-4, 100.0, 12345, 0.1


def scene(name):
    import viennaray_amd as vr
    from helpers import trench2d, trench3d
    if name == "trench2d":
        gd, p, n = trench2d()
        t = vr.TraceDisk(2)
        t.setGeometry(p, n, gd)
        t.setSourceDirection(vr.TraceDirection.POS_Y)
        t.setBoundaryConditions([vr.BoundaryCondition.PERIODIC_BOUNDARY] * 2)
    else:
        gd, p, n = trench3d()
        t = vr.TraceDisk(3)
        t.setGeometry(p, n, gd)
        t.setBoundaryConditions([vr.BoundaryCondition.PERIODIC_BOUNDARY] * 3)
    t.setParticleType(vr.DiffuseParticle(STICKING, "flux"))
    t.setRngSeed(SEED)
    w = np.exp(np.random.default_rng(5).uniform(np.log(0.05), np.log(3.0), size=len(p))).astype(np.float32)
    return t, p, n, w


def timed_apply(t):
    t.setRunNumber(1)
    t0 = time.perf_counter()
    t.apply()
    wall = (time.perf_counter() - t0) * 1e3
    i = t.getRayTraceInfo()
    return dict(apply_wall_ms=wall, device_ms=i.timeTrace * 1e3, gen_kernel_ms=i.timeGenKernel * 1e3,
                trace_kernel_ms=i.timeTraceKernel * 1e3, rays=int(i.numRays), mode=t.traceMode())


def child(variant, name, R, rayfile):
    t, p, n, w = scene(name)
    out = dict(variant=variant, scene=name, R=R)
    if variant == "dump":      # the rays of run number 1, for the host-ray baseline
        t.setNumberOfRaysPerPoint(R)
        t.setSurfaceSource(p, n, w, AREA, OFFSET)
        total, step = len(p) * R, 1 << 24
        parts = [t.debugSurfaceSourceSample(np.arange(a, min(a + step, total), dtype=np.uint64), SEED + 1)
                 for a in range(0, total, step)]
        np.savez(rayfile, org=np.concatenate([q[0] for q in parts]), dir=np.concatenate([q[1] for q in parts]),
                 w=np.concatenate([q[2] for q in parts]), k=np.concatenate([q[3] for q in parts]))
        out["rays"] = total
    elif variant == "host":    # (VR_LIB_PATH = the baseline library)
        z = np.load(rayfile)
        org, d, wr, k = z["org"], z["dir"], z["w"], z["k"]

        def once():
            t0 = time.perf_counter()
            t.setHostRays(org, d, k, weights=wr, sourceArea=AREA)
            s = (time.perf_counter() - t0) * 1e3
            r = timed_apply(t)
            r["set_ms"] = s
            r["total_ms"] = s + r["apply_wall_ms"]
            return r
        once()
        out.update(once())
        out["flux_sum"] = float(t.getFluxF64().sum())
    elif variant == "sampler":  # a vectorised numpy sampler of a tenth of the rays (the host work the device source saves)
        m = max(1, len(p) * R // 10)
        rng = np.random.default_rng(1)
        t0 = time.perf_counter()
        j = np.arange(m) // R
        nn = n[j] / np.linalg.norm(n[j], axis=1, keepdims=True)
        r1, r2 = rng.random(m, dtype=np.float32), rng.random(m, dtype=np.float32)
        ct = np.sqrt(r2)
        st = np.sqrt(np.maximum(0, 1 - ct * ct))
        phi = 2 * np.pi * r1
        s = np.copysign(np.float32(1), nn[:, 2])
        a = -1 / (s + nn[:, 2])
        b = nn[:, 0] * nn[:, 1] * a
        tt = np.stack([1 + s * nn[:, 0] ** 2 * a, s * b, -s * nn[:, 0]], 1)
        b2 = np.stack([b, s + nn[:, 1] ** 2 * a, -nn[:, 1]], 1)
        d = nn * ct[:, None] + tt * (np.cos(phi) * st)[:, None] + b2 * (np.sin(phi) * st)[:, None]
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        org = p[j] + nn * np.float32(OFFSET)
        out.update(rays=m, sampler_ms=(time.perf_counter() - t0) * 1e3, checksum=float(d.sum() + org.sum()))
    else:                       # "device"
        t.setNumberOfRaysPerPoint(R)

        def once():
            t0 = time.perf_counter()
            t.setSurfaceSource(p, n, w, AREA, OFFSET)
            s = (time.perf_counter() - t0) * 1e3
            r = timed_apply(t)
            r["set_ms"] = s
            r["total_ms"] = s + r["apply_wall_ms"]
            return r
        once()
        out.update(once())
        out["flux_sum"] = float(t.getFluxF64().sum())
    print(json.dumps(out), flush=True)


def driver(name, R, rounds):
    import tempfile
    rayfile = os.path.join(tempfile.gettempdir(), "surface_rays_%s_%d_%d.npz" % (name, R, os.getpid()))
    baseline = os.environ.get("VR_BASELINE_LIB") or os.path.join(ROOT, "viennaray_amd", "libviennaray_amd.so")

    def run(variant, env_extra, limit):
        env = dict(os.environ)
        env.update(env_extra)
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "child", variant, name,
                            str(R), rayfile], env=env, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:   # a GPU step failed: nothing more is started
            sys.stdout.write(r.stderr[-3000:])
            sys.exit(r.returncode)
    run("dump", {}, 300)
    run("sampler", {}, 200)
    for _ in range(rounds):
        run("device", {}, 200)
        run("host", {"VR_LIB_PATH": baseline}, 300)
    os.remove(rayfile)


if __name__ == "__main__":
    if sys.argv[1] == "child":
        child(sys.argv[2], sys.argv[3], int(sys.argv[4]), sys.argv[5])
    else:
        driver(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 3)
