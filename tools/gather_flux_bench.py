#!/usr/bin/env python3
"""What gatherFlux costs (Trace.gatherFlux: rays cast from every primitive, generated, walked, weighed and summed in one
kernel), on C2's plane of 10^6 disks and on tests/golden/data/trenchGrid3D.dat, at K = 64 and 256 samples per primitive,
against the same walk fed from memory: castRays over rays of the same law (a primitive's centre, a cosine direction
about its normal, primitive by primitive, lifted off it by 1e-3 gridDelta), followBoundaries on.  The cast is timed over
at most `cast_rays` rays — N x K rays of 24 bytes would not fit at K = 256 — and both rates are recorded side by side; no
ratio is formed (the cast's figure on the plane is not understood).  One process, device events on torch's stream around the
calls, warm-up rounds first, median over the rounds.  Writes profiles/gather_flux_bench.json and prints it as one line.
usage: tools/gather_flux_bench.py [rounds=5] [warmup=2] [cast_rays=16777216]"""
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


def scenes():
    pts, nrm = vr.io.plane_grid(1000, 1.0)
    yield "C2 plane, 10^6 disks", pts.astype(np.float32), nrm.astype(np.float32), 1.0
    gd, pts, nrm = trench3d()
    yield "trenchGrid3D", pts.astype(np.float32), nrm.astype(np.float32), float(gd)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def cosine_rays(pts, nrm, k, limit):
    """k cosine directions about the normal of each of the first limit // k primitives, on the device, primitive by primitive"""
    n = max(1, min(pts.shape[0], limit // k))
    p = torch.from_numpy(pts[:n]).cuda().repeat_interleave(k, 0)
    m = torch.nn.functional.normalize(torch.from_numpy(nrm[:n]).cuda(), dim=1).repeat_interleave(k, 0)
    g = torch.Generator(device="cuda").manual_seed(1)
    r1, r2 = torch.rand(n * k, device="cuda", generator=g), torch.rand(n * k, device="cuda", generator=g)
    helper = torch.where(m[:, :1].abs() < 0.9, torch.tensor([[1.0, 0, 0]], device="cuda"), torch.tensor([[0, 1.0, 0]], device="cuda"))
    u = torch.nn.functional.normalize(torch.linalg.cross(m, helper), dim=1)
    v = torch.linalg.cross(m, u)
    s, phi = torch.sqrt(1 - r2), 2 * np.pi * r1
    d = (s * torch.cos(phi))[:, None] * u + (s * torch.sin(phi))[:, None] * v + torch.sqrt(r2)[:, None] * m
    return p.contiguous(), d.contiguous(), m.contiguous()


def case(name, pts, nrm, gd, rounds, warmup, cast_rays):
    t = vr.TraceDisk(3)
    t.setGeometry(pts, nrm, gd)
    t.setBoundaryConditions([vr.BoundaryCondition.REFLECTIVE_BOUNDARY] * 3)
    t.setParticleType(vr.DiffuseParticle(1.0, "flux"))
    t.setNumberOfRaysFixed(1_000_000)
    t.setUseRandomSeeds(False)
    t.setRngSeed(12345)
    t.applyPrepare()
    n = int(pts.shape[0])
    out = dict(scene=name, primitives=n, rounds=rounds, samples={})
    for k in (64, 256):
        ms = [timed(lambda: t.gatherFlux(k))[0] for _ in range(warmup + rounds)][warmup:]
        flux = t.gatherFlux(k)
        # the cast's rays leave from 1e-3 gridDelta above the centres (tools/cast_rays_bench.py's scattered rays); the same
        # rays from the centres themselves, as the gather starts its own, are timed once beside them
        o0, d, m = cosine_rays(pts, nrm, k, cast_rays)
        o = (o0 + 1e-3 * gd * m).contiguous()
        cms = [timed(lambda: t.castRays(o, d))[0] for _ in range(warmup + rounds)][warmup:]
        in_plane_ms = [timed(lambda: t.castRays(o0, d))[0] for _ in range(2)][1]
        del o0, m
        g_rate = n * k / (statistics.median(ms) * 1e-3) / 1e6
        c_rate = o.shape[0] / (statistics.median(cms) * 1e-3) / 1e6
        out["samples"][str(k)] = dict(
            gather_ms=dict(median=round(statistics.median(ms), 3), min=round(min(ms), 3)),
            gather_msamples_per_s=round(g_rate, 1), mean_flux=round(float(flux.mean()), 5),
            cast_rays=int(o.shape[0]), cast_ms=dict(median=round(statistics.median(cms), 3), min=round(min(cms), 3)),
            cast_mrays_per_s=round(c_rate, 1), cast_from_the_centres_ms=round(in_plane_ms, 3))
        del o, d
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rounds = int(args[0]) if len(args) > 0 else 5
    warmup = int(args[1]) if len(args) > 1 else 2
    cast_rays = int(args[2]) if len(args) > 2 else 1 << 24
    cases = [case(name, p, nr, gd, rounds, warmup, cast_rays) for name, p, nr, gd in scenes()]
    res = dict(tool="gather_flux_bench", device=torch.cuda.get_device_name(0), cases=cases)
    with open(os.path.join(ROOT, "profiles", "gather_flux_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
