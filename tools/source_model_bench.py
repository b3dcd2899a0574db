#!/usr/bin/env python3
"""Source model: one apply() whose rays a device source model samples in the generator, against the SAME rays handed over
through setHostRays (origins, directions, draw counts and — for a weighted source — weights), on the same build.  Every
measurement is a child process (a warm-up round, then REPEATS timed rounds of setter + apply, of which the median is
taken per figure); the two alternate, `rounds` times.  Reported per child: the setter's wall time, apply()'s wall time
(prepare + launch + finish), their sum, and the generator and trace kernel times of the library's own events.  The
driver checks that both ways give the same flux and counters, and writes every line into one JSON file.
usage: tools/source_model_bench.py <beam|rejection> <rays> [rounds] [out.json]           (driver)
       tools/source_model_bench.py child <variant> <source> <rays> <rayfile>             (one measurement)"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SEED, STICKING, REPEATS = 12345, 0.1, 5

# the test sources of tests/test_source_models.py: a beam with spread; the same behind a rejection loop, with a weight
BEAM_CORE = """
template <int D, class Draw>
__device__ static void beam(const SourceCtx &s, Draw &&draw, V3 &org, V3 &dir, float a, float b) {
  const float r1 = canon_f32(draw()), r2 = canon_f32(draw());
  org = mk(0.f, 0.f, 0.f);
  setc(org, s.rayDir, s.srcCoord);
  setc(org, s.firstDir, s.bbLo[s.firstDir] + (s.bbHi[s.firstDir] - s.bbLo[s.firstDir]) * r1);
  if (D == 3)
    setc(org, s.secondDir, s.bbLo[s.secondDir] + (s.bbHi[s.secondDir] - s.bbLo[s.secondDir]) * r2);
  const float r3 = canon_f32(draw()), r4 = canon_f32(draw());
  dir = mk(0.f, 0.f, 0.f);
  setc(dir, s.firstDir, a * (2.f * r3 - 1.f));
  setc(dir, s.secondDir, D == 3 ? b * (2.f * r4 - 1.f) : 0.f);
  setc(dir, s.rayDir, s.posNeg);
  vnormalize(dir);
}
"""
SOURCES = {
    "beam": (BEAM_CORE + """
struct VrUserSource {
  static constexpr bool kHasWeight = false;
  template <int D, class Draw>
  __device__ static void sample(const SourceCtx &s, unsigned long long, Draw &&draw, V3 &org, V3 &dir, float &) {
    beam<D>(s, draw, org, dir, s.params[0], s.params[1]);
  }
};
""", (0.3, 0.2), False),
    "rejection": (BEAM_CORE + """
struct VrUserSource {
  static constexpr bool kHasWeight = true;
  template <int D, class Draw>
  __device__ static void sample(const SourceCtx &s, unsigned long long, Draw &&draw, V3 &org, V3 &dir, float &weight) {
    float r = 0.f;
    for (int k = 0; k < 8; ++k) {
      r = canon_f32(draw());
      if (r < s.params[0])
        break;
    }
    beam<D>(s, draw, org, dir, s.params[1], s.params[2]);
    weight = 0.25f + r;
  }
};
""", (0.3, 0.3, 0.2), True),
}


def scene():
    import viennaray_amd as vr
    from helpers import trench3d
    gd, p, n = trench3d()
    t = vr.TraceDisk(3)
    t.setGeometry(p, n, gd)
    t.setBoundaryConditions([vr.BoundaryCondition.PERIODIC_BOUNDARY] * 3)
    t.setParticleType(vr.DiffuseParticle(STICKING, "flux"))
    t.setRngSeed(SEED)
    return vr, t


def timed_round(t, setter):
    """setter + apply of run number 1"""
    t0 = time.perf_counter()
    setter()
    s = (time.perf_counter() - t0) * 1e3
    t.setRunNumber(1)
    t0 = time.perf_counter()
    t.apply()
    wall = (time.perf_counter() - t0) * 1e3
    i = t.getRayTraceInfo()
    return dict(set_ms=s, apply_wall_ms=wall, total_ms=s + wall, device_ms=i.timeTrace * 1e3,
                gen_kernel_ms=i.timeGenKernel * 1e3, trace_kernel_ms=i.timeTraceKernel * 1e3, rays=int(i.numRays),
                mode=t.traceMode(), traced=int(i.totalRaysTraced), geometryHits=int(i.geometryHits))


def median_rounds(once):
    """a warm-up round, then the median of REPEATS rounds per figure (the counters are the same in all of them)"""
    once()
    rows = [once() for _ in range(REPEATS)]
    return {key: (float(np.median([r[key] for r in rows])) if key.endswith("_ms") else rows[-1][key]) for key in rows[-1]}


def child(variant, source, rays, rayfile):
    vr, t = scene()
    text, params, weighted = SOURCES[source]
    model = vr.SourceModel(source, text, params=params, numRays=rays, hasWeight=weighted)
    out = dict(variant=variant, source=source)
    if variant == "dump":      # the rays of run number 1, for the host-ray path (the first registration compiles the module)
        t0 = time.perf_counter()
        t.setSource(model)
        out["register_ms"] = (time.perf_counter() - t0) * 1e3
        step = 1 << 22
        parts = [t.debugUserSourceSample(np.arange(a, min(a + step, rays), dtype=np.uint64), SEED + 1)
                 for a in range(0, rays, step)]
        np.savez(rayfile, org=np.concatenate([q[0] for q in parts]), dir=np.concatenate([q[1] for q in parts]),
                 w=np.concatenate([q[2] for q in parts]), k=np.concatenate([q[3] for q in parts]))
        out["rays"] = rays
    elif variant == "host":
        z = np.load(rayfile)
        org, d, w, k = z["org"], z["dir"], z["w"], z["k"]
        once = lambda: timed_round(t, lambda: t.setHostRays(org, d, k, weights=w if weighted else None))  # noqa: E731
        out.update(median_rounds(once))
        out["flux_sum"] = float(t.getFluxF64().sum())
    else:                      # "device"
        t.setSource(model)     # (registered: the timed setter below finds the loaded module, as every later time step does)
        once = lambda: timed_round(t, lambda: t.setSource(model))  # noqa: E731
        out.update(median_rounds(once))
        out["flux_sum"] = float(t.getFluxF64().sum())
    print(json.dumps(out), flush=True)


def driver(source, rays, rounds, outfile):
    import tempfile
    rayfile = os.path.join(tempfile.gettempdir(), "source_model_rays_%s_%d_%d.npz" % (source, rays, os.getpid()))
    lines = []

    def run(variant, limit):
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "child", variant,
                            source, str(rays), rayfile], capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:   # a GPU step failed: nothing more is started
            sys.stdout.write(r.stderr[-3000:])
            sys.exit(r.returncode or 1)
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
    run("dump", 300)
    for _ in range(rounds):
        run("device", 200)
        run("host", 300)
    os.remove(rayfile)
    dev = [q for q in lines if q["variant"] == "device"]
    host = [q for q in lines if q["variant"] == "host"]
    same = all(a[key] == b[key] for a, b in zip(dev, host) for key in ("flux_sum", "rays", "mode", "traced", "geometryHits"))
    med = lambda rows, key: float(np.median([q[key] for q in rows]))  # noqa: E731
    summary = dict(source=source, rays=rays, rounds=rounds, same_result=same,
                   **{"%s_%s" % (name, key): med(rows, key) for name, rows in (("device", dev), ("host", host))
                      for key in ("set_ms", "apply_wall_ms", "total_ms", "gen_kernel_ms", "trace_kernel_ms")})
    print(json.dumps(dict(summary=summary)), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(outfile)), exist_ok=True)
    previous = []
    if os.path.exists(outfile):
        previous = [q for q in json.load(open(outfile)) if q["summary"]["source"] != source]
    json.dump(previous + [dict(summary=summary, runs=lines)], open(outfile, "w"), indent=1)
    if not same:
        sys.exit("the two ways disagree")


if __name__ == "__main__":
    if sys.argv[1] == "child":
        child(sys.argv[2], sys.argv[3], int(sys.argv[4]), sys.argv[5])
    else:
        driver(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 3,
               sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "source_model_bench.json"))
