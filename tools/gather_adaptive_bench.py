#!/usr/bin/env python3
"""What the gather to a target error costs and saves (Trace.gatherFluxAdaptive / gatherPathsAdaptive), on
tests/golden/data/trenchGrid3D.dat and on the 10^6-disk rippled sheet (bench.py's C2_rippled).  Per scene, for gatherFlux at
cosinePower 1 and 8 and for specular gatherPaths at reflectivity 0.7:
  1. the adaptive call at target 5 %, 64 .. 4096 samples: time, totalSamples, rounds, unconverged, the histogram of
     samplesUsed, and the share of primitives that meet the rule;
  2. the fixed-K call it is set against: the smallest power-of-two K at which the same rule (gather_converged on the sums
     of chunks [0, K / 64), evaluated in numpy as tests/test_gather_adaptive_host.py does) is met by at least that share of
     primitives — 4096 if none is — with its time and its samples;
  3. gatherFluxSums over chunks [0, 4) against gatherFlux(256): what the second sum and the chunk offset cost.
One process, device events on torch's stream around the calls (the adaptive call's per-round waits for its one word are
inside), warm-up rounds first, median over the rounds.  Writes profiles/gather_adaptive_bench.json and prints it as one line.
usage: tools/gather_adaptive_bench.py [rounds=5] [warmup=2]"""
import json
import os
import statistics
import sys

import numpy as np
import torch  # (before the tracing library: one HIP runtime for both)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import viennaray_amd as vr  # noqa: E402
from gather_paths_bench import med, scenes, timed, tracer  # noqa: E402

TARGET, LO, HI = 0.05, 64, 4096
LEVELS = [LO << r for r in range(7)]


def converged(s1, s2, K, rel):
    """vr_gather.hpp's gather_converged (abs = 0), one float64 operation at a time"""
    k = np.float64(K)
    m1 = s1.astype(np.float64) * np.float64(2.0 ** -40) / k
    m2 = s2.astype(np.float64) * np.float64(2.0 ** -28) / k
    v = m2 - m1 * m1
    v = np.where(v > 0, v, 0.0)
    tol = np.float64(np.float32(rel)) * m1
    return v / (k - 1.0) <= tol * tol


def settings(t):
    yield ("gatherFlux_n1", lambda K: t.gatherFlux(K), lambda c, K: t.gatherFluxSums(0, c, K),
           lambda: t.gatherFluxAdaptive(TARGET, minSamples=LO, maxSamples=HI, returnInfo=True))
    yield ("gatherFlux_n8", lambda K: t.gatherFlux(K, cosinePower=8.0), lambda c, K: t.gatherFluxSums(0, c, K, cosinePower=8.0),
           lambda: t.gatherFluxAdaptive(TARGET, minSamples=LO, maxSamples=HI, cosinePower=8.0, returnInfo=True))
    yield ("gatherPaths_specular_rho0.7", lambda K: t.gatherPaths(K, reflectivity=0.7),
           lambda c, K: t.gatherPathsSums(0, c, K, reflectivity=0.7),
           lambda: t.gatherPathsAdaptive(TARGET, reflectivity=0.7, minSamples=LO, maxSamples=HI, returnInfo=True))


def case(name, pts, nrm, gd, rounds, warmup):
    t = tracer(pts, nrm, gd)
    n = int(pts.shape[0])
    out = dict(scene=name, primitives=n, rounds=rounds, target=TARGET, min_samples=LO, max_samples=HI, settings={})
    for key, fixed, sums, adaptive in settings(t):
        ms = med(adaptive, rounds, warmup)
        flux, err, used, info = adaptive()
        used = used.cpu().numpy().astype(np.int64)
        share = 1.0 - info["unconverged"] / n
        e = dict(adaptive_ms=ms, total_samples=info["totalSamples"], rounds=info["rounds"], unconverged=info["unconverged"],
                 share_met=round(share, 5), mean_flux=round(float(flux.mean()), 5),
                 samples_used={str(k): int((used == k).sum()) for k in LEVELS},
                 msamples_per_s=round(info["totalSamples"] / (ms["median"] * 1e-3) / 1e6, 1))
        shares, pick = {}, HI
        for K in LEVELS:
            s1, s2 = sums(K // 64, K)
            shares[str(K)] = round(float(converged(s1.cpu().numpy(), s2.cpu().numpy(), K, TARGET).mean()), 5)
        for K in LEVELS:
            if shares[str(K)] >= share:
                pick = K
                break
        fms = med(lambda: fixed(pick), rounds, warmup)
        e["fixed"] = dict(samples=pick, total_samples=pick * n, ms=fms, share_met_by_K=shares,
                          msamples_per_s=round(pick * n / (fms["median"] * 1e-3) / 1e6, 1))
        e["adaptive_over_fixed_time"] = round(ms["median"] / fms["median"], 3)
        e["adaptive_over_fixed_samples"] = round(info["totalSamples"] / (pick * n), 4)
        out["settings"][key] = e
    out["sums_K256"] = dict(gather_flux_ms=med(lambda: t.gatherFlux(256), rounds, warmup),
                            gather_flux_sums_ms=med(lambda: t.gatherFluxSums(0, 4, 256), rounds, warmup),
                            gather_paths_ms=med(lambda: t.gatherPaths(256, reflectivity=0.7), rounds, warmup),
                            gather_paths_sums_ms=med(lambda: t.gatherPathsSums(0, 4, 256, reflectivity=0.7), rounds, warmup))
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rounds = int(args[0]) if len(args) > 0 else 5
    warmup = int(args[1]) if len(args) > 1 else 2
    cases = [case(name, p, nr, gd, rounds, warmup) for name, p, nr, gd in scenes()]
    res = dict(tool="gather_adaptive_bench", device=torch.cuda.get_device_name(0), cases=cases)
    with open(os.path.join(ROOT, "profiles", "gather_adaptive_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
