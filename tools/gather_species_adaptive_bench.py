#!/usr/bin/env python3
"""What one walk saves when every species runs to its own target error (Trace.gatherSpeciesAdaptive: the rounds of the
adaptive gather once for up to four species, a mask of the species still sampling per listed primitive), on the two scenes
of tools/gather_species_bench.py — tests/golden/data/trenchGrid3D.dat and the 10^6-disk rippled sheet — specular and
diffuse, maxBounces 64, target 0.05 for every species, minSamples 64, maxSamples 4096, the species A .. D of that tool.
Per scene and reflection, in the same run: the species call at S = 2 (A, B) and S = 4 (A .. D), and the four separate
gatherAngularAdaptive calls of the same species — the gather's own kernels, whose text and registers this commit leaves as
they were.  The bar of S species is the SUM of their separate calls.  One process, device events on torch's stream around
the calls, warm-up rounds first, the rounds interleaved (every call once per round), median over the rounds; `spread` is the
largest (max - min) / median among the separate calls, what a saving has to exceed to mean anything: `undercuts_bar` says
whether 1 - species / bar does.  Every row of flux, stdErr and samples of the species call is checked against its separate
call, bit for bit; walkedSamples / sum of totalSamples is the share of the separate calls' samples that is still walked.
Then, in gather_species_bench's setting (K = 64 and 256, S = 2 and 4), the time of gatherSpeciesSums — the existing call
whose kernels gained the list branch — and of the fixed-K gatherSpecies, whose kernels did not.  With --sums-only only that
part runs: pointed at a build of the parent commit (VR_LIB_PATH) it gives the figure to compare with, and --parent-sums
merges such a file into the result as species_sums_parent with the ratios beside it.
Writes profiles/gather_species_adaptive_bench.json (or the path given as the third argument) and prints it as one line.
usage: tools/gather_species_adaptive_bench.py [rounds=5] [warmup=2] [out.json] [--sums-only] [--parent-sums parent.json]"""
import json
import os
import statistics
import sys

import torch  # (before the tracing library: one HIP runtime for both)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import viennaray_amd as vr  # noqa: E402
from gather_angular_bench import scenes, tracer, timed  # noqa: E402
from gather_species_bench import SPECIES, KINDS, BOUNCES, SAMPLES, stats  # noqa: E402

TARGET, MIN_SAMPLES, MAX_SAMPLES = 0.05, 64, 4096
COUNTS = (2, 4)


def interleaved(calls, rounds, warmup):
    ms = {key: [] for key in calls}
    for rnd in range(warmup + rounds):
        for key, fn in calls.items():
            dt, _ = timed(fn)
            if rnd >= warmup:
                ms[key].append(dt)
    return {key: stats(v) for key, v in ms.items()}


def adaptive_case(t, rounds, warmup):
    r = {}
    for kind in KINDS:
        kw = dict(reflection=kind, maxBounces=BOUNCES, minSamples=MIN_SAMPLES, maxSamples=MAX_SAMPLES)
        calls = {"species_%d" % s: (lambda s=s: t.gatherSpeciesAdaptive(TARGET, SPECIES[:s], **kw)) for s in COUNTS}
        calls.update({"separate_%d" % i: (lambda i=i: t.gatherAngularAdaptive(TARGET, **SPECIES[i], **kw)) for i in range(len(SPECIES))})
        st = interleaved(calls, rounds, warmup)
        ones = [t.gatherAngularAdaptive(TARGET, **SPECIES[i], returnInfo=True, **kw) for i in range(len(SPECIES))]
        spread = max(st["separate_%d" % i]["spread"] for i in range(len(SPECIES)))
        res = dict(separate_spread=spread, separate_ms=[st["separate_%d" % i] for i in range(len(SPECIES))],
                   separate_info=[o[3] for o in ones])
        for s in COUNTS:
            flux, err, used, info = t.gatherSpeciesAdaptive(TARGET, SPECIES[:s], returnInfo=True, **kw)
            same = all(bool((flux[i] == ones[i][0]).all() and (err[i] == ones[i][1]).all() and (used[i] == ones[i][2]).all())
                       for i in range(s))
            same = same and info["totalSamples"] == [ones[i][3]["totalSamples"] for i in range(s)]
            bar = sum(st["separate_%d" % i]["median"] for i in range(s))
            ratio = st["species_%d" % s]["median"] / bar
            res["S%d" % s] = dict(species_ms=st["species_%d" % s], sum_of_separate_ms=round(bar, 4), species_over_sum=round(ratio, 4),
                                  undercuts_bar=bool(1.0 - ratio > spread), rows_same_bits=same, info=info,
                                  walked_over_total=round(info["walkedSamples"] / sum(info["totalSamples"]), 4))
        r[kind.name.lower()] = res
        print("#", kind.name.lower(), {k: v["species_over_sum"] for k, v in res.items() if k.startswith("S")}, flush=True)
    return r


def sums_case(t, rounds, warmup):
    r = {}
    for k in SAMPLES:
        rk = {}
        for kind in KINDS:
            kw = dict(reflection=kind, maxBounces=BOUNCES)
            calls = {"sums_%d" % s: (lambda s=s: t.gatherSpeciesSums(0, k // 64, k, SPECIES[:s], **kw)) for s in COUNTS}
            calls["fixed_4"] = lambda: t.gatherSpecies(k, SPECIES, **kw)
            rk[kind.name.lower()] = interleaved(calls, rounds, warmup)
        r[str(k)] = rk
        print("# sums", k, {kind: {c: v["median"] for c, v in rk[kind].items()} for kind in rk}, flush=True)
    return r


def main():
    args = sys.argv[1:]
    sums_only = "--sums-only" in args
    parent = None
    if "--parent-sums" in args:
        i = args.index("--parent-sums")
        with open(args[i + 1]) as f:
            parent = json.load(f)
        del args[i:i + 2]
    args = [a for a in args if a != "--sums-only"]
    rounds = int(args[0]) if len(args) > 0 else 5
    warmup = int(args[1]) if len(args) > 1 else 2
    path = args[2] if len(args) > 2 else os.path.join(ROOT, "profiles", "gather_species_adaptive_bench.json")
    cases = []
    for name, pts, nrm, gd in scenes():
        t = tracer(pts, nrm, gd)
        out = dict(scene=name, primitives=int(pts.shape[0]), rounds=rounds, max_bounces=BOUNCES)
        if not sums_only:
            out.update(target=TARGET, min_samples=MIN_SAMPLES, max_samples=MAX_SAMPLES, adaptive=adaptive_case(t, rounds, warmup))
        out["species_sums"] = sums_case(t, rounds, warmup)
        cases.append(out)
    library = "a build named by VR_LIB_PATH" if os.environ.get("VR_LIB_PATH") else "this build"
    res = dict(tool="gather_species_adaptive_bench", device=torch.cuda.get_device_name(0), library=library, cases=cases)
    if parent is not None:  # the same calls timed against a build of the parent commit: this build's median over the parent's
        for mine, theirs in zip(cases, parent["cases"]):
            mine["species_sums_parent"] = theirs["species_sums"]
            mine["species_sums_over_parent"] = {
                k: {kind: {c: round(v["median"] / theirs["species_sums"][k][kind][c]["median"], 4) for c, v in calls.items()}
                    for kind, calls in kinds.items()} for k, kinds in mine["species_sums"].items()}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
