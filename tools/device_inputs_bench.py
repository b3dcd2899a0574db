#!/usr/bin/env python3
"""What the host round trip of a time step's INPUTS costs, on a geometry that stays where it is:

  coverage step      set one global vector (the coverages), apply(collect=False), getFluxTensor
  re-emission step   setSurfaceSource with weights computed from the flux tensor, apply(collect=False), getFluxTensor

  the host way     the coverages / weights are computed on the device (they are functions of the flux tensor), downloaded,
                   and handed to the host entry points (vr_set_global_data, vr_set_surface_source)
  the device way   the tensors go in where they are (vr_set_global_data_device, vr_set_surface_source_device)

on a plane of 10^6 disks and on trenchGrid3D.dat, 10^6 rays a step.  A step is timed as a whole on the wall clock, ending
with torch.cuda.synchronize(); the two ways alternate step by step in one process, on two contexts with the same scene.
The driver runs that measurement in fresh processes, alternating between this tree's library and the parent commit's
(viennaray_amd/libviennaray_amd_prev.so, built by tools/build_prev.sh; it has the host way only), RUNS times each, and
prints one JSON line: per scene and step the median of every run, as min .. max over the runs.
usage: tools/device_inputs_bench.py [runs=8] [steps=20] [warmup=3]      (tools/device_inputs_bench.py --child ... : one run)"""
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch  # (before the tracing library: one HIP runtime for both)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import viennaray_amd as vr  # noqa: E402
from helpers import trench3d  # noqa: E402

PREV = os.path.join(ROOT, "viennaray_amd", "libviennaray_amd_prev.so")
AREA, OFFSET = 100.0, 1e-4
RAYS = 1_000_000


def scene(name):
    if name == "plane_1e6":
        pts, nrm = vr.io.plane_grid(1000, 1.0)
        return 1.0, pts, nrm
    return trench3d()


def tracer(gd, p, n):
    t = vr.TraceDisk(3)
    t.setGeometry(p, n, gd)
    t.setBoundaryConditions([vr.BoundaryCondition.PERIODIC_BOUNDARY] * 3)
    t.setParticleType(vr.CoverageStickingParticle(0.5, "flux"))
    t.setNumberOfRaysFixed(RAYS)
    t.setUseRandomSeeds(False)
    t.setRngSeed(12345)
    return t


def set_vector(t, v):
    """vector 0 of the global data alone (Trace.setGlobalVector; an older library's front-end has setGlobalData only)"""
    if hasattr(t, "setGlobalVector"):
        t.setGlobalVector(0, v)
    else:
        t.setGlobalData([v])


def coverage_step(t, cov_d, on_device):
    t0 = time.perf_counter()
    set_vector(t, cov_d if on_device else cov_d.cpu().numpy())
    t.setRunNumber(1)
    t.apply(collect=False)
    f = t.getFluxTensor()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, f


def emission_step(t, P, N, flux_d, on_device):
    t0 = time.perf_counter()
    w = torch.clamp(flux_d * 0.0625, max=1.0) + 0.125
    if on_device:
        t.setSurfaceSource(P[0], N[0], w, AREA, OFFSET)
    else:
        t.setSurfaceSource(P[1], N[1], w.cpu().numpy(), AREA, OFFSET)
    t.setRunNumber(1)
    t.apply(collect=False)
    f = t.getFluxTensor()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, f


def child(steps, warmup):
    have_device = hasattr(vr.load(), "vr_set_global_data_device")
    ways = ["host", "device"] if have_device else ["host"]
    out = {}
    for name in ("plane_1e6", "trenchGrid3D"):
        gd, p, n = scene(name)
        P, N = (torch.from_numpy(p).cuda(), p), (torch.from_numpy(n).cuda(), n)
        per_point = max(1, RAYS // len(p))
        rows = {}
        for kind in ("coverage", "emission"):
            ctx = {w: tracer(gd, p, n) for w in ways}
            cov = {w: torch.full((len(p),), 0.25, dtype=torch.float32, device="cuda") for w in ways}
            flux = {}
            if kind == "emission":  # the first pass, once: the weights are functions of its flux
                for w in ways:
                    ctx[w].apply(collect=False)
                    flux[w] = ctx[w].getFluxTensor()
                    ctx[w].setNumberOfRaysPerPoint(per_point)
            ms = {w: [] for w in ways}
            last = {}
            for k in range(warmup + steps):
                for w in ways:
                    if kind == "coverage":
                        dt, f = coverage_step(ctx[w], cov[w], w == "device")
                        cov[w] = cov[w] * 0.5 + torch.clamp(f * 0.03125, max=1.0) * 0.5
                    else:
                        dt, f = emission_step(ctx[w], P, N, flux[w], w == "device")
                    last[w] = f
                    if k >= warmup:
                        ms[w].append(dt)
            torch.cuda.synchronize()
            rows[kind] = {w: round(statistics.median(ms[w]), 4) for w in ways}
            if have_device:
                rows[kind]["bit_equal"] = bool(torch.equal(last["host"], last["device"]))
        out[name] = dict(disks=int(len(p)), median_ms=rows)
    print(json.dumps(out), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(int(sys.argv[2]), int(sys.argv[3]))
    runs = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    warmup = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    libs = [("head", None)] + ([("parent", PREV)] if os.path.exists(PREV) else [])
    res = {name: [] for name, _ in libs}
    for _ in range(runs):
        for name, path in libs:  # interleaved: head, parent, head, parent, ...
            env = dict(os.environ)
            env.pop("VR_LIB_PATH", None)
            if path:
                env["VR_LIB_PATH"] = path
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(steps), str(warmup)], env=env,
                               capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                sys.stderr.write(p.stderr[-3000:])
                raise SystemExit(f"{name}: the measuring process failed ({p.returncode})")
            res[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
    table = []
    for sc in res["head"][0]:
        for kind in ("coverage", "emission"):
            def span(lib, way):
                v = [r[sc]["median_ms"][kind][way] for r in res[lib]]
                return dict(min=min(v), median=round(statistics.median(v), 4), max=max(v))
            row = dict(scene=sc, disks=res["head"][0][sc]["disks"], step=kind, head_device=span("head", "device"),
                       head_host=span("head", "host"),
                       bit_equal=all(r[sc]["median_ms"][kind]["bit_equal"] for r in res["head"]))
            if "parent" in res:
                row["parent_host"] = span("parent", "host")
                row["device_not_slower_than_parent"] = row["head_device"]["median"] <= row["parent_host"]["max"]
            row["device_not_slower_than_host"] = row["head_device"]["median"] <= row["head_host"]["median"]
            table.append(row)
    print(json.dumps(dict(tool="device_inputs_bench", device=torch.cuda.get_device_name(0), runs=runs, steps=steps,
                          rays=RAYS, rows=table)), flush=True)


if __name__ == "__main__":
    main()
