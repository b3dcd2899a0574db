#!/usr/bin/env python3
"""Cost of the flux statistics (Trace.setCalculateFluxError): Mrays/s of one apply() with statistics off and on, and —
if a build of the parent commit lies next to the library (tools/build_prev.sh: libviennaray_amd_prev.so) — the
statistics-off rate of that build, in one session on one card.

Workloads: trenchGrid3D.dat at sticking 0.1 and 1.0 (2000 rays per point), and the flat and the rippled (half a grid
cell) million-disk sheets of tools/case_bench.py at sticking 0.1 (10 rays per point).  Every measurement is a child
process: one warm-up apply, then three timed ones, of which the median is reported with the smallest and the largest
(the run-to-run spread); the rate is rays / the apply's device time (generator + trace + gather, the library's events).
The variants of a workload run one after the other, the parent build between the two of this build.
Writes profiles/flux_statistics_bench.json.
usage: tools/flux_error_bench.py [out.json]                       (driver)
       tools/flux_error_bench.py child <workload> <off|on>        (one measurement; VR_LIB_PATH picks the build)"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PREV = os.path.join(ROOT, "viennaray_amd", "libviennaray_amd_prev.so")
WORKLOADS = ("trench3d_0.1", "trench3d_1.0", "plane1000_0.1", "ripple1000_0.1")
STEPS = 3


def scene(workload):
    import viennaray_amd as vr
    from helpers import trench3d
    name, sticking = workload.rsplit("_", 1)
    if name == "trench3d":
        gd, p, n = trench3d()
        rpp = 2000
    else:
        side, amp = 1000, (0.5 if name.startswith("ripple") else 0.0)
        ax = np.arange(side) - (side - 1) / 2.0
        x, y = np.meshgrid(ax, ax, indexing="ij")
        wave = 4.0
        z = amp * np.sin(x / wave) * np.cos(y / wave)
        n = np.stack([-amp / wave * np.cos(x / wave) * np.cos(y / wave), amp / wave * np.sin(x / wave) * np.sin(y / wave),
                      np.ones_like(x)], -1).reshape(-1, 3)
        n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
        p = np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32)
        gd, rpp = 1.0, 10
    t = vr.TraceDisk(3)
    t.setGeometry(p, n, gd)
    t.setBoundaryConditions([vr.BoundaryCondition.PERIODIC_BOUNDARY] * 3)
    t.setParticleType(vr.DiffuseParticle(float(sticking), "flux"))
    t.setNumberOfRaysPerPoint(rpp)
    t.setRngSeed(12345)
    return t


def child(workload, variant):
    t = scene(workload)
    if variant == "on":
        t.setCalculateFluxError(True)
    rows = []
    for step in range(STEPS + 1):   # (the first one warms up: scene build, buffers, code objects)
        t.setRunNumber(1)
        t.apply(collect=False)
        i = t.getRayTraceInfo()
        rows.append(dict(device_ms=i.timeTrace * 1e3, trace_kernel_ms=i.timeTraceKernel * 1e3, rays=int(i.numRays)))
    rows = rows[1:]
    rate = sorted(r["rays"] / r["device_ms"] * 1e-3 for r in rows)
    out = dict(workload=workload, variant=variant, build="parent" if os.environ.get("VR_LIB_PATH") else "this", mode=t.traceMode(),
               rays=rows[0]["rays"], mrays_per_s=rate[len(rate) // 2], mrays_min=rate[0], mrays_max=rate[-1],
               trace_kernel_ms=float(np.median([r["trace_kernel_ms"] for r in rows])),
               flux_sum=float(t.getFluxF64().sum()))
    if variant == "on":
        rel = t.getFluxRelativeError()
        out["median_relative_error"] = float(np.median(rel[np.isfinite(rel)]))
    print(json.dumps(out), flush=True)


def driver(outfile):
    lines = []

    def run(workload, variant, lib=None):
        env = dict(os.environ)
        env.pop("VR_LIB_PATH", None)
        if lib:
            env["VR_LIB_PATH"] = lib
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "child", workload, variant],
                           capture_output=True, text=True, env=env)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:   # a GPU step failed: nothing more is started
            sys.stdout.write(r.stderr[-3000:])
            sys.exit(r.returncode or 1)
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
    have_prev = os.path.exists(PREV)
    for w in WORKLOADS:
        run(w, "off")
        if have_prev:
            run(w, "off", PREV)
        run(w, "on")
    summary = []
    for w in WORKLOADS:
        row = {q["build"] + "_" + q["variant"]: q for q in lines if q["workload"] == w}
        off, on, prev = row["this_off"], row["this_on"], row.get("parent_off")
        s = dict(workload=w, off_mrays=off["mrays_per_s"], on_mrays=on["mrays_per_s"], off_mode=off["mode"], on_mode=on["mode"],
                 on_over_off=on["mrays_per_s"] / off["mrays_per_s"],
                 off_spread=(off["mrays_max"] - off["mrays_min"]) / off["mrays_per_s"], same_flux=off["flux_sum"] == on["flux_sum"])
        if prev:
            s.update(parent_off_mrays=prev["mrays_per_s"], off_over_parent=off["mrays_per_s"] / prev["mrays_per_s"],
                     parent_spread=(prev["mrays_max"] - prev["mrays_min"]) / prev["mrays_per_s"], parent_mode=prev["mode"],
                     same_flux_as_parent=prev["flux_sum"] == off["flux_sum"])
        summary.append(s)
        print(json.dumps(dict(summary=s)), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(outfile)), exist_ok=True)
    json.dump(dict(summary=summary, runs=lines), open(outfile, "w"), indent=1)
    if not all(s["same_flux"] for s in summary):
        sys.exit("statistics on changed the flux")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "child":
        child(sys.argv[2], sys.argv[3])
    else:
        driver(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "flux_statistics_bench.json"))
