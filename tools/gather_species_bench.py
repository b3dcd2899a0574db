#!/usr/bin/env python3
"""What one walk for several species saves (Trace.gatherSpecies: up to four species weighed along one set of traced paths,
gather_species_kernel), on the two scenes of tools/gather_angular_bench.py — tests/golden/data/trenchGrid3D.dat and the
10^6-disk rippled sheet — at K = 64 and 256 samples per primitive, specular and diffuse, maxBounces 64.  The species:
  A  reflectivity 0.7;                     B  reflectivity 0.5 with the yield Y rising from 0.5 to 3;
  C  reflectivity 0.9 with R falling from 1 to 0.2;   D  reflectivity 0.7 with the source law L from c^3.
Per scene, K and reflection, in the same run: the species call at S = 1 (A), 2 (A, B) and 4 (A .. D), and the four separate
gatherAngular calls of the same species — the gather's own kernel, whose text and registers this commit leaves as they
were.  The bar of S species is the SUM of their separate calls.  One process, device events on torch's stream around the
calls, warm-up rounds first, the rounds interleaved (every call once per round), median over the rounds; `spread` is the
largest (max - min) / median among the separate calls, what a saving has to exceed to mean anything.  Every row of the
species call is checked against its separate call, bit for bit.  Writes profiles/gather_species_bench.json (or the path
given as the third argument) and prints it as one line.
usage: tools/gather_species_bench.py [rounds=5] [warmup=2] [out.json]"""
import json
import os
import statistics
import sys

import numpy as np
import torch  # (before the tracing library: one HIP runtime for both)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import viennaray_amd as vr  # noqa: E402
from gather_angular_bench import scenes, tracer, timed  # noqa: E402

SAMPLES = (64, 256)
KINDS = (vr.GatherReflection.SPECULAR, vr.GatherReflection.DIFFUSE)
BOUNCES = 64
SPECIES = [dict(reflectivity=0.7),
           dict(reflectivity=0.5, yieldLaw=np.linspace(0.5, 3.0, 5).astype(np.float32)),
           dict(reflectivity=0.9, reflectivityLaw=np.linspace(1.0, 0.2, 5).astype(np.float32)),
           dict(reflectivity=0.7, sourceLaw=(np.linspace(0.0, 1.0, 5) ** 3).astype(np.float32))]
COUNTS = (1, 2, 4)


def stats(ms):
    m = statistics.median(ms)
    return dict(median=round(m, 4), min=round(min(ms), 4), spread=round((max(ms) - min(ms)) / m, 4))


def case(name, pts, nrm, gd, rounds, warmup):
    t = tracer(pts, nrm, gd)
    out = dict(scene=name, primitives=int(pts.shape[0]), rounds=rounds, max_bounces=BOUNCES, samples={})
    for k in SAMPLES:
        r = {}
        for kind in KINDS:
            kw = dict(reflection=kind, maxBounces=BOUNCES)
            calls = {"species_%d" % s: (lambda s=s: t.gatherSpecies(k, SPECIES[:s], **kw)) for s in COUNTS}
            calls.update({"separate_%d" % i: (lambda i=i: t.gatherAngular(k, **SPECIES[i], **kw)) for i in range(len(SPECIES))})
            ms = {key: [] for key in calls}
            for rnd in range(warmup + rounds):
                for key, fn in calls.items():
                    dt, _ = timed(fn)
                    if rnd >= warmup:
                        ms[key].append(dt)
            st = {key: stats(v) for key, v in ms.items()}
            rows = t.gatherSpecies(k, SPECIES, **kw)
            same = all(bool((rows[i] == t.gatherAngular(k, **SPECIES[i], **kw)).all()) for i in range(len(SPECIES)))
            spread = max(st["separate_%d" % i]["spread"] for i in range(len(SPECIES)))
            res = dict(rows_same_bits=same, separate_spread=spread, separate_ms=[st["separate_%d" % i] for i in range(len(SPECIES))])
            for s in COUNTS:
                bar = sum(st["separate_%d" % i]["median"] for i in range(s))
                res["S%d" % s] = dict(species_ms=st["species_%d" % s], sum_of_separate_ms=round(bar, 4),
                                      species_over_sum=round(st["species_%d" % s]["median"] / bar, 4))
            r[kind.name.lower()] = res
        out["samples"][str(k)] = r
    return out


def main():
    args = sys.argv[1:]
    rounds = int(args[0]) if len(args) > 0 else 5
    warmup = int(args[1]) if len(args) > 1 else 2
    path = args[2] if len(args) > 2 else os.path.join(ROOT, "profiles", "gather_species_bench.json")
    cases = [case(name, p, nr, gd, rounds, warmup) for name, p, nr, gd in scenes()]
    res = dict(tool="gather_species_bench", device=torch.cuda.get_device_name(0), cases=cases)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
