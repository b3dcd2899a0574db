#!/usr/bin/env python3
"""What carrying an ion's energy costs, and what the cut saves (Trace.gatherEnergy: gatherAngular with E0 and the product of
the retentions per path, a kernel of its own — gather_energy_kernel — with the energy tables staged in LDS), on the two
scenes of tools/gather_paths_bench.py — tests/golden/data/trenchGrid3D.dat and the 10^6-disk rippled sheet — at K = 64 and
256 samples per primitive, specular and diffuse, reflectivity 0.7, maxBounces 64.  Per scene, K and reflection, in the same
run and with the same arguments:
  (a) angular    gatherAngular with an all-ones reflectivity law: the PATH 3 kernel, whose text and registers this commit
                 leaves as they were;
      ones       gatherEnergy with an all-ones energyYield (M = 256) on top of it: the same bits, every look-up made;
  (b) cut_off    gatherEnergy under energyYield = [0, 0, 1], a retention law falling from 1 to 0.3 and the source quantiles
                 {30, 60, 100} of energyMax = 100, energyCut = False;
      cut_on     the same with energyCut = True: the same bits (checked in the run), fewer segments.
One process, device events on torch's stream around the calls, the variants interleaved round by round, warm-up rounds
first, median over the rounds; `spread` is (max - min) / median of the gatherAngular rounds, what a ratio has to exceed to
mean anything.  The share of paths the cut ended and the segments walked per sample come from the counters of a
-DVR_DIAG build of the library (make -C viennaray_amd/csrc diag), run once per setting in a child process; without that
library they are left out.  Writes profiles/gather_energy_bench.json (or the path given as the third argument) and prints
it as one line.
usage: tools/gather_energy_bench.py [rounds=5] [warmup=2] [out.json]"""
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

SAMPLES = (64, 256)
KINDS = (vr.GatherReflection.SPECULAR, vr.GatherReflection.DIFFUSE)
RHO, BOUNCES = 0.7, 64
DIAG_LIB = os.path.join(ROOT, "viennaray_amd", "libviennaray_amd_diag.so")
ANGULAR = dict(reflectivityLaw=np.ones(256, np.float32))
ONES = dict(energyYield=np.ones(256, np.float32), energyMax=100.0, sourceQuantiles=[30.0, 60.0, 100.0],
            retentionLaw=np.linspace(1.0, 0.3, 8).astype(np.float32))
ION = dict(energyYield=[0.0, 0.0, 1.0], energyMax=100.0, sourceQuantiles=[30.0, 60.0, 100.0],
           retentionLaw=np.linspace(1.0, 0.3, 8).astype(np.float32))


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


def variants(t, k, kw):
    return {"angular": lambda: t.gatherAngular(k, **ANGULAR, **kw),
            "ones": lambda: t.gatherEnergy(k, **ONES, **ANGULAR, **kw),
            "cut_off": lambda: t.gatherEnergy(k, energyCut=False, **ION, **kw),
            "cut_on": lambda: t.gatherEnergy(k, energyCut=True, **ION, **kw)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def interleaved(fns, rounds, warmup):
    """every variant once per round, in turn, so that a drift of the clocks meets all of them alike"""
    ms = {name: [] for name in fns}
    for r in range(warmup + rounds):
        for name, fn in fns.items():
            dt = timed(fn)[0]
            if r >= warmup:
                ms[name].append(dt)
    out = {}
    for name, v in ms.items():
        m = statistics.median(v)
        out[name] = dict(median=round(m, 4), min=round(min(v), 4), spread=round((max(v) - min(v)) / m, 4))
    return out


def diag_child():
    """under the -DVR_DIAG library: every setting once; the library prints one line of counters per call on stderr"""
    for name, pts, nrm, gd in scenes():
        t = tracer(pts, nrm, gd)
        for k in SAMPLES:
            for kind in KINDS:
                kw = dict(reflectivity=RHO, reflection=kind, maxBounces=BOUNCES)
                for variant, fn in variants(t, k, kw).items():
                    sys.stderr.write("diag case %s | %d | %s | %s\n" % (name, k, kind.name.lower(), variant))
                    sys.stderr.flush()
                    fn()
                    torch.cuda.synchronize()


def lane_counters():
    """{(scene, K, reflection, variant): (rounds, segments, paths)} from a child process under the diag library, or {}"""
    if not os.path.exists(DIAG_LIB):
        return {}
    env = dict(os.environ, VR_LIB_PATH=DIAG_LIB)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--diag-child"], env=env, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-2000:])
        return {}
    out, case = {}, None
    for line in p.stderr.splitlines():
        m = re.match(r"diag case (.*) \| (\d+) \| (\S+) \| (\S+)$", line)
        if m:
            case = (m.group(1), int(m.group(2)), m.group(3), m.group(4))
        m = re.match(r"diag gather paths: rounds (\d+) segments (\d+) paths (\d+)$", line)
        if m and case:
            out[case] = tuple(int(v) for v in m.groups())
    return out


def cut_share(t, k, kw, prims=16, per=16):
    """the share of paths the cut ends, from the one-path walk over a few primitives spread over the scene"""
    n = int(t._L.vr_num_primitives(t._h))
    ended = total = 0
    for prim in np.linspace(0, n - 1, prims).astype(int):
        for s in range(per):
            p = t.debugGatherEnergyPath(int(prim), s * (k // per), dict(ION, energyCut=True), maxVertices=0, **kw)
            ended += int(p["end"] == vr.GatherEnd.ENERGY)
            total += 1
    return round(ended / total, 4)


def case(name, pts, nrm, gd, rounds, warmup, lanes):
    t = tracer(pts, nrm, gd)
    out = dict(scene=name, primitives=int(pts.shape[0]), rounds=rounds, reflectivity=RHO, max_bounces=BOUNCES, samples={})
    for k in SAMPLES:
        r = {}
        for kind in KINDS:
            kw = dict(reflectivity=RHO, reflection=kind, maxBounces=BOUNCES)
            fns = variants(t, k, kw)
            ms = interleaved(fns, rounds, warmup)
            same_ones = bool((fns["ones"]() == fns["angular"]()).all())
            on, off = fns["cut_on"](), fns["cut_off"]()
            same_cut = bool((on.view(torch.int32) == off.view(torch.int32)).all())
            row = dict(angular_ms=ms["angular"], ones_ms=ms["ones"], cut_off_ms=ms["cut_off"], cut_on_ms=ms["cut_on"],
                       ones_same_bits=same_ones, cut_same_bits=same_cut,
                       ones_over_angular=round(ms["ones"]["median"] / ms["angular"]["median"], 4),
                       cut_on_over_cut_off=round(ms["cut_on"]["median"] / ms["cut_off"]["median"], 4),
                       cut_share_of_paths=cut_share(t, k, kw), mean_flux_ion=round(float(on.mean()), 5))
            for variant in ("angular", "ones", "cut_off", "cut_on"):
                c = lanes.get((name, k, kind.name.lower(), variant))
                if c:
                    row["segments_per_sample_" + variant] = round(c[1] / c[2], 4)
            r[kind.name.lower()] = row
        out["samples"][str(k)] = r
    return out


def main():
    if "--diag-child" in sys.argv:
        return diag_child()
    args = sys.argv[1:]
    rounds = int(args[0]) if len(args) > 0 else 5
    warmup = int(args[1]) if len(args) > 1 else 2
    path = args[2] if len(args) > 2 else os.path.join(ROOT, "profiles", "gather_energy_bench.json")
    lanes = lane_counters()
    cases = [case(name, p, nr, gd, rounds, warmup, lanes) for name, p, nr, gd in scenes()]
    res = dict(tool="gather_energy_bench", device=torch.cuda.get_device_name(0), diag_counters=bool(lanes), cases=cases,
               not_measured="triangle meshes and 2-D scenes at a size where occupancy matters")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
