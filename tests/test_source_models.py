"""Device source models (vr_register_source_model / vr_set_source_model): a user Source compiled into the ray generator.

Three test sources, written with + - * / sqrt and the library's own conversions only, so that numpy float32 restates them
bit for bit: Beam (4 draws, no weight), Rejection (a draw count that differs from lane to lane, a weight) and Long (Beam,
but one ray in 64 first burns 160 draws: past the 156 outputs of the streaming engine).  The device sample must equal the
restatement; an apply() must equal the same rays handed over through setHostRays — accumulators, counters and trace mode —
and the oracle fed with those rays.
"""
import os
import subprocess

import numpy as np
import pytest

import viennaray_amd as vr
from viennaray_amd import capi
from oracle import pyoracle as po
from helpers import ROOT, l2_rel

REF = vr.BoundaryCondition.REFLECTIVE_BOUNDARY
CSRC = os.path.join(ROOT, "viennaray_amd", "csrc")
NEW_SYMBOLS = ("vr_register_source_model", "vr_set_source_model", "vr_set_source_model_table_device",
               "vr_debug_user_source_sample")
INFO_KEYS = ("numRays", "totalRaysTraced", "nonGeometryHits", "geometryHits", "particleHits", "boundaryHits",
             "reflections", "raysTerminated", "warning", "error", "rngFullStates", "bvhRefits")
ORACLE_KEYS = ("numRays", "totalRaysTraced", "nonGeometryHits", "geometryHits", "particleHits", "boundaryHits",
               "reflections", "raysTerminated")
FLUX_TOL = 1e-4  # the standing tolerance of test_gpu_parity.py
FACADE_FLAGS = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include",
                "-I", os.path.join(ROOT, "include", "viennaray_amd"), "-I", os.path.join(ROOT, "include")]
FACADE_SRC = os.path.join(ROOT, "tests", "aux", "facade_source_model.cpp")
RAYS = 4096
SEED = 4711          # setRngSeed; the kernel seed of run number 1 is SEED + 1
A, B, ACCEPT = 0.3, 0.2, 0.3
SAMPLE_IDX = (0, 1, 3, 63, 64, 67, 4095)

# ---------------------------------------------------------------------------------------------------------------------
# the test sources
# ---------------------------------------------------------------------------------------------------------------------
# what Beam, Rejection, Long and Table share: the origin uniform on the source face of the bounding box from two draws (the
# second one unused in 2-D), the direction normalize(a (2 r - 1), b (2 r - 1), posNeg) on the axes (first, second, ray)
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
BEAM = BEAM_CORE + """
struct VrUserSource {
  static constexpr bool kHasWeight = false;
  template <int D, class Draw>
  __device__ static void sample(const SourceCtx &s, unsigned long long, Draw &&draw, V3 &org, V3 &dir, float &) {
    beam<D>(s, draw, org, dir, s.params[0], s.params[1]);
  }
};
"""
REJECTION = BEAM_CORE + """
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
"""
LONG = BEAM_CORE + """
struct VrUserSource {
  static constexpr bool kHasWeight = false;
  template <int D, class Draw>
  __device__ static void sample(const SourceCtx &s, unsigned long long idx, Draw &&draw, V3 &org, V3 &dir, float &) {
    if (idx % 64ull == 3ull)
      for (int k = 0; k < 160; ++k)
        (void)draw();
    beam<D>(s, draw, org, dir, s.params[0], s.params[1]);
  }
};
"""
TABLE = BEAM_CORE + """
struct VrUserSource {
  static constexpr bool kHasWeight = false;
  template <int D, class Draw>
  __device__ static void sample(const SourceCtx &s, unsigned long long idx, Draw &&draw, V3 &org, V3 &dir, float &) {
    beam<D>(s, draw, org, dir, s.table[idx % s.tableCount], s.params[1]);
  }
};
"""
TEXTS = {"beam": BEAM, "rejection": REJECTION, "long": LONG, "table": TABLE}
HAS_WEIGHT = {"beam": False, "rejection": True, "long": False, "table": False}


def _model(kind, table=None, numRays=RAYS):
    params = (ACCEPT, A, B) if kind == "rejection" else (A, B)
    return vr.SourceModel(kind, TEXTS[kind], params=params, table=table, numRays=numRays, hasWeight=HAS_WEIGHT[kind])


# ---------------------------------------------------------------------------------------------------------------------
# the numpy restatement
# ---------------------------------------------------------------------------------------------------------------------
F = np.float32


def _canon(raw):
    """canon_f32 (vr_rng.hpp): float(u64) * 2^-64, clamped below 1"""
    f = F(np.uint64(raw)) * F(2.0 ** -64)
    return F(0.99999994) if f >= F(1.0) else f


class Frame:
    """what SourceCtx tells the sources: the adjusted box and the source frame of POS_Y (2-D) / POS_Z (3-D)
    (rayUtil.hpp getTraceSettings: {ray, first, second, max side, -1})"""

    def __init__(self, D, box):
        self.D = D
        self.lo, self.hi = box[0].astype(F), box[1].astype(F)
        self.ray, self.first, self.second = (1, 0, 2) if D == 2 else (2, 0, 1)
        self.posNeg = F(-1.0)
        self.src = self.hi[self.ray]


def _beam(fr, draw, a, b):
    r1, r2 = _canon(draw()), _canon(draw())
    org = np.zeros(3, F)
    org[fr.ray] = fr.src
    org[fr.first] = fr.lo[fr.first] + (fr.hi[fr.first] - fr.lo[fr.first]) * r1
    if fr.D == 3:
        org[fr.second] = fr.lo[fr.second] + (fr.hi[fr.second] - fr.lo[fr.second]) * r2
    r3, r4 = _canon(draw()), _canon(draw())
    d = np.zeros(3, F)
    d[fr.first] = F(a) * (F(2.0) * r3 - F(1.0))
    d[fr.second] = F(b) * (F(2.0) * r4 - F(1.0)) if fr.D == 3 else F(0.0)
    d[fr.ray] = fr.posNeg
    n = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])  # (vnormalize: vdot's order)
    return org, d / n


def restate(kind, fr, idx, raw, table=None):
    """(origin, direction, weight, draws) of ray idx; raw: the engine's first outputs (at least 170)"""
    k = [0]

    def draw():
        k[0] += 1
        return raw[k[0] - 1]

    w = F(1.0)
    a = F(A)
    if kind == "rejection":
        r = F(0.0)
        for _ in range(8):
            r = _canon(draw())
            if r < F(ACCEPT):
                break
        w = F(0.25) + r
    elif kind == "long" and idx % 64 == 3:
        for _ in range(160):
            draw()
    elif kind == "table":
        a = F(table[idx % len(table)])
    org, d = _beam(fr, draw, a, F(B))
    return org, d, w, k[0]


def restate_all(kind, fr, indices, outputs, table=None):
    O, Dr, W, K = [], [], [], []
    for i in indices:
        o, d, w, k = restate(kind, fr, int(i), outputs(int(i)), table)
        O.append(o)
        Dr.append(d)
        W.append(w)
        K.append(k)
    return np.array(O, F), np.array(Dr, F), np.array(W, F), np.array(K, np.uint32)


def _oracle_outputs(seed):
    return lambda idx: po.mt64_outputs(po.tea3(idx, seed), 176)


# ---------------------------------------------------------------------------------------------------------------------
# no GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_source_model_entry_points_are_declared_exported_and_bound():
    txt = open(os.path.join(ROOT, "include", "viennaray_amd.h")).read()
    L = vr.load()
    for name in NEW_SYMBOLS:
        assert name + "(" in txt, name
        assert hasattr(L, name), name
        assert name in capi.SIGNATURES, name
        res, args = capi.SIGNATURES[name]
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert len(capi.SIGNATURES["vr_set_source_model"][1]) == 7
    assert len(capi.SIGNATURES["vr_debug_user_source_sample"][1]) == 8
    for method in ("registerSourceModel", "setSourceModelTable", "debugUserSourceSample"):
        assert callable(getattr(vr.Trace, method, None)), method


def test_source_model_argument_validation():
    m = vr.SourceModel("beam", BEAM, params=[0.1] * 16, table=np.arange(5, dtype=np.float32), numRays=7)
    assert m.params.dtype == np.float32 and m.params.size == 16 and m.table.size == 5 and m.numRays == 7 and not m.hasWeight
    assert vr.SourceModel("beam", BEAM).table is None
    assert vr.SourceModel("beam", BEAM, table=[1.0, 2.0]).table.dtype == np.float32  # (a list of numbers is a host table)
    with pytest.raises(ValueError, match="params"):
        vr.SourceModel("beam", BEAM, params=[0.0] * 17)
    with pytest.raises(ValueError, match="params"):
        vr.SourceModel("beam", BEAM, params=np.zeros((2, 2)))
    with pytest.raises(ValueError, match="dtype"):
        vr.SourceModel("beam", BEAM, table=np.arange(5, dtype=np.float64))
    with pytest.raises(ValueError, match="dtype"):
        vr.SourceModel("beam", BEAM, table=np.arange(5, dtype=np.int32))
    with pytest.raises(ValueError, match="shape"):
        vr.SourceModel("beam", BEAM, table=np.zeros((2, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="numRays"):
        vr.SourceModel("beam", BEAM, numRays=1 << 32)
    with pytest.raises(ValueError, match="source"):
        vr.SourceModel("beam", "")


def test_cpp_facade_names_the_source_model_methods():
    hdr = open(os.path.join(ROOT, "include", "viennaray_amd", "viennaray.hpp")).read()
    assert "int registerSourceModel(const std::string &name, const std::string &source, bool hasWeight" in hdr
    assert "void setSourceModel(int id, const std::vector<float> &params" in hdr
    p = subprocess.run(["g++", "-fsyntax-only"] + FACADE_FLAGS + [FACADE_SRC], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]


@pytest.mark.parametrize("D", [2, 3])
def test_restatements_draw_what_they_should(D):
    """the restatements on the oracle's engine (mt64_outputs, uniform_float): the conversion is the library's, Beam draws 4,
    Rejection 5 .. 12 with the geometric split of its accept rate, Long 164 for exactly one ray in 64"""
    fr = Frame(D, np.array([[-1.0, -2.0, -3.0], [5.0, 7.0, 11.0]], F))
    out = _oracle_outputs(SEED + 1)
    raw = out(17)
    assert np.array_equal(np.array([_canon(v) for v in raw], F).view(np.uint32), po.uniform_float(raw).view(np.uint32))
    idx = np.arange(RAYS)
    o, d, w, k = restate_all("beam", fr, idx, out)
    assert (k == 4).all() and (w == 1).all()
    assert np.allclose(np.linalg.norm(d.astype(np.float64), axis=1), 1.0, atol=1e-6)
    assert (o[:, fr.ray] == fr.src).all() and (o[:, fr.first] >= fr.lo[fr.first]).all() and (o[:, fr.first] <= fr.hi[fr.first]).all()
    if D == 2:
        assert (o[:, 2] == 0).all() and (d[:, 2] == 0).all()
    _, _, w, k = restate_all("rejection", fr, idx, out)
    assert k.min() == 5 and k.max() == 12 and len(np.unique(k)) == 8        # every loop length occurs
    assert len(np.unique(k[:64])) >= 4                                       # ... within one wave
    first = (k == 5).mean()
    assert abs(first - ACCEPT) < 0.03                                        # (accepted at the first draw: +- 4 sigma of 4096)
    assert (w[k < 12] < F(0.25) + F(ACCEPT)).all() and (w >= F(0.25)).all()
    ol, dl, _, k = restate_all("long", fr, idx, out)
    assert ((k >= 156) == (idx % 64 == 3)).all() and (k[idx % 64 == 3] == 164).all() and (k[idx % 64 != 3] == 4).all()
    assert int((k >= 156).sum()) * 64 == RAYS
    same = idx % 64 != 3  # (the other rays are Beam's)
    assert np.array_equal(ol[same], o[same]) and np.array_equal(dl[same], d[same])
    assert not np.array_equal(ol[~same], o[~same])


def _compile_source_module(tmp_path, text, has_weight):
    """a stand-in for the translation unit vr_register_source_model writes — the same defines and include, without its
    layout asserts — parsed for gfx950 (no device needed): it says that a text is well-formed against the source-module
    section of vr_trace.hip and that the section's own static_asserts fire, nothing about the generated unit itself"""
    (tmp_path / "source.hpp").write_text(text)
    tu = tmp_path / "module.hip"
    tu.write_text("#define VR_USER_MODULE 1\n#define VR_USER_SOURCE_MODULE 1\n"
                  f"#define VR_USER_SOURCE_HAS_WEIGHT {int(has_weight)}\n"
                  f"#define VR_USER_SOURCE_FILE \"{tmp_path / 'source.hpp'}\"\n#include <cstddef>\n"
                  f"#include \"{CSRC}/vr_trace.hip\"\n")
    hipcc = os.environ.get("VR_HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "--genco", "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "-I", CSRC, str(tu)],
                       capture_output=True, text=True)
    return r.returncode, r.stdout + r.stderr


def test_source_texts_parse_and_the_weight_flag_is_checked(tmp_path):
    """the four test sources are well-formed source modules; kHasWeight must be what the registration said"""
    for kind, text in TEXTS.items():
        rc, out = _compile_source_module(tmp_path, text, HAS_WEIGHT[kind])
        assert rc == 0, (kind, out)
    rc, out = _compile_source_module(tmp_path, REJECTION, False)
    assert rc != 0 and "kHasWeight differs from the VR_SOURCE_HAS_WEIGHT flag given at registration" in out


# ---------------------------------------------------------------------------------------------------------------------
# GPU: helpers
# ---------------------------------------------------------------------------------------------------------------------
def _torch():
    import torch
    return torch


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def cache(tmp_path_factory):
    """one code-object cache for the module: each source model is compiled once"""
    return str(tmp_path_factory.mktemp("vr_source_cache"))


@pytest.fixture(autouse=True)
def _use_cache(request, monkeypatch):
    if "cache" in request.fixturenames:
        monkeypatch.setenv("VR_CACHE_DIR", request.getfixturevalue("cache"))


def _scene(D):
    """a plane with a step: the upper half three cells above the lower one, the wall between them (more disks than the
    LDS-resident kernel takes, so that an absorbing particle runs an absorbing kernel)"""
    if D == 3:
        nx = ny = 36
        x, y = np.meshgrid(np.arange(nx, dtype=F), np.arange(ny, dtype=F), indexing="ij")
        x, y = x.ravel(), y.ravel()
        p = np.stack([x, y, np.where(x < nx // 2, F(3.0), F(0.0))], axis=1)
        n = np.tile(np.array([[0, 0, 1]], F), (p.shape[0], 1))
        wy, wz = np.meshgrid(np.arange(ny, dtype=F), np.array([0.5, 1.5, 2.5], F), indexing="ij")
        wall = np.stack([np.full(wy.size, nx // 2 - 0.5, F), wy.ravel(), wz.ravel()], axis=1)
        p = np.concatenate([p, wall]).astype(F)
        n = np.concatenate([n, np.tile(np.array([[1, 0, 0]], F), (wall.shape[0], 1))]).astype(F)
        return 1.0, p, n
    nx = 1500
    x = np.arange(nx, dtype=F)
    p = np.stack([x, np.where(x < nx // 2, F(3.0), F(0.0))], axis=1)
    n = np.tile(np.array([[0, 1]], F), (nx, 1))
    wall = np.stack([np.full(3, nx // 2 - 0.5, F), np.array([0.5, 1.5, 2.5], F)], axis=1)
    p = np.concatenate([p, wall]).astype(F)
    n = np.concatenate([n, np.tile(np.array([[1, 0]], F), (3, 1))]).astype(F)
    return 1.0, p, n


def _tracer(D, sticking=0.1, rays=None):
    gd, p, n = _scene(D)
    t = vr.TraceDisk(D)
    t.setGeometry(p, n, gd)
    t.setBoundaryConditions([REF] * D)
    if D == 2:
        t.setSourceDirection(vr.TraceDirection.POS_Y)
    if rays:
        t.setNumberOfRaysFixed(rays)
    t.setRngSeed(SEED)
    t.setParticleType(vr.DiffuseParticle(sticking, "flux"))
    return t


def _frame(t, D):
    t.applyPrepare()
    return Frame(D, t.getBoundingBox())


def _run(t):
    """apply with run number 1: (int64 accumulators, counters, trace mode)"""
    torch = _torch()
    acc = torch.zeros(t._n * t.numData(), dtype=torch.int64, device="cuda")
    t.bindFluxAccumulators(acc.data_ptr(), acc.numel())
    t.setRunNumber(1)
    t.apply()
    torch.cuda.synchronize()
    i = t.getRayTraceInfo()
    return acc.cpu().numpy().copy(), {k: int(getattr(i, k)) for k in INFO_KEYS}, t.traceMode()


def _same(a, b, what=""):
    assert a[1] == b[1], (what, a[1], b[1])
    assert a[2] == b[2], (what, "trace mode", a[2], b[2])
    assert np.array_equal(a[0], b[0]), (what, int((a[0] != b[0]).sum()))


_RAYS = {}


def _rays(kind, D, fr, table=None):
    """the restated rays of a whole apply, computed once per source and dimension and shared"""
    key = (kind, D)
    if key not in _RAYS:
        _RAYS[key] = restate_all(kind, fr, np.arange(RAYS), _oracle_outputs(SEED + 1), table)
    return _RAYS[key]


def _host_tracer(D, sticking, kind, fr):
    """the same rays through setHostRays"""
    o, d, w, k = _rays(kind, D, fr)
    h = _tracer(D, sticking)
    h.setHostRays(o, d, k, weights=w if HAS_WEIGHT[kind] else None)
    return h


# ---------------------------------------------------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("kind", ["beam", "rejection", "long"])
def test_sample_parity(kind, D, cache):
    """the generator's sample against the restatement on the DEVICE engine's outputs (vr_debug_rng_outputs): origin,
    direction, weight and draw count bit for bit"""
    t = _tracer(D)
    t.setSource(_model(kind))
    fr = _frame(t, D)
    idx = np.concatenate([np.array(SAMPLE_IDX), np.random.default_rng(9).integers(0, RAYS, 256)]).astype(np.uint64)
    seed = SEED + 1
    o, d, w, k = t.debugUserSourceSample(idx, seed)
    ro, rd, rw, rk = restate_all(kind, fr, idx, lambda i: t.debugRngOutputs(i, seed, 176))
    assert np.array_equal(k, rk), (k[:8], rk[:8])
    assert np.array_equal(o.view(np.uint32), ro.view(np.uint32))
    assert np.array_equal(d.view(np.uint32), rd.view(np.uint32))
    assert np.array_equal(w.view(np.uint32), rw.view(np.uint32))
    # ... and the device engine is the oracle's
    assert np.array_equal(t.debugRngOutputs(67, seed, 176), _oracle_outputs(seed)(67))


@pytest.mark.gpu
@pytest.mark.parametrize("sticking", [1.0, 0.1])
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("kind", ["beam", "rejection", "long"])
def test_equals_the_host_ray_path_and_the_oracle(kind, D, sticking, cache):
    """apply() with the source model against a second tracer given the restated rays through setHostRays: accumulators,
    every counter and the trace mode identical; and against the oracle with those rays: counters identical, flux within
    the standing 1e-4"""
    t = _tracer(D, sticking)
    t.setSource(_model(kind))
    fr = _frame(t, D)
    got = _run(t)
    assert got[1]["numRays"] == RAYS
    _same(got, _run(_host_tracer(D, sticking, kind, fr)), "host rays")
    if sticking == 1.0 and not HAS_WEIGHT[kind]:
        assert got[2] in (1, 2), got[2]  # a weightless source keeps the absorbing kernels
    if sticking < 1.0 and kind == "long":
        assert got[1]["rngFullStates"] > 0, got[1]  # rays that go on behind 164 draws: the tracer rebuilds the full state
    o, d, w, k = _rays(kind, D, fr)
    gd, p, n = _scene(D)
    orc = po.Oracle()
    if D == 2:  # (the oracle takes three columns)
        p, n = np.pad(p, ((0, 0), (0, 1))), np.pad(n, ((0, 0), (0, 1)))
    orc.set_disks(p, n, gd, D)
    orc.set_boundary_conditions([po.REFLECTIVE] * D)
    if D == 2:
        orc.set_source_direction(po.POS_Y)
    orc.set_particle(po.DIFFUSE, sticking)
    orc.set_rng_seed(SEED)
    orc.set_host_rays(o, d, weights=w if HAS_WEIGHT[kind] else None)
    orc.set_host_ray_draws(k)
    orc.set_lazy_rng(True)
    orc.apply(po.max_threads())
    oi = orc.info()
    assert {key: got[1][key] for key in ORACLE_KEYS} == {key: oi[key] for key in ORACLE_KEYS}
    flux = got[0].astype(np.float64) * 2.0 ** -40
    assert l2_rel(flux, orc.flux()) <= FLUX_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("kind,sticking", [("rejection", 0.1), ("long", 1.0)])
def test_two_halves_of_the_ray_range_sum_to_the_whole(kind, sticking, cache):
    """vr_set_ray_range: the sample depends on the global index only (a count that splits a wave)"""
    rays = RAYS + 37
    t = _tracer(3, sticking)
    t.setSource(_model(kind, numRays=rays))
    whole = _run(t)
    half = rays // 2
    t.setRayRange(0, half)
    a = _run(t)
    t.setRayRange(half, rays - half)
    b = _run(t)
    assert np.array_equal(a[0] + b[0], whole[0])
    for key in ("totalRaysTraced", "nonGeometryHits", "geometryHits", "boundaryHits", "reflections", "raysTerminated",
                "rngFullStates"):
        assert a[1][key] + b[1][key] == whole[1][key], key
    t.setRayRange(0, 0)
    _same(_run(t), whole, "the whole range again")


@pytest.mark.gpu
def test_ray_count_follows_source_random_without_a_count_of_its_own(cache):
    t = _tracer(3, 1.0, rays=1000)
    t.setSource(_model("beam", numRays=0))
    assert _run(t)[1]["numRays"] == 1000
    t.setNumberOfRaysPerPoint(2)
    assert _run(t)[1]["numRays"] == 2 * t._n


@pytest.mark.gpu
def test_device_table_equals_host_table(cache):
    torch = _torch()
    table = np.linspace(0.05, 0.6, 37).astype(F)
    h = _tracer(3)
    h.setSource(_model("table", table=table))
    fr = _frame(h, 3)
    host = _run(h)
    d = _tracer(3)
    d.setSource(_model("table", table=_dev(table)))
    _same(_run(d), host, "device table")
    # the table is really read: the restatement with it, and another table gives other rays
    idx = np.array(SAMPLE_IDX, dtype=np.uint64)
    o, dr, w, k = d.debugUserSourceSample(idx, SEED + 1)
    ro, rd, rw, rk = restate_all("table", fr, idx, _oracle_outputs(SEED + 1), table)
    assert np.array_equal(dr.view(np.uint32), rd.view(np.uint32)) and np.array_equal(o.view(np.uint32), ro.view(np.uint32))
    # refusals: each raises ValueError and the previous table stays
    for bad in (torch.from_numpy(table), _dev(table.astype(np.float64)), _dev(np.repeat(table, 2))[::2],
                _dev(np.stack([table, table]))):
        with pytest.raises(ValueError):
            d.setSource(_model("table", table=bad))
        if bad.device.type != "cpu":
            with pytest.raises(ValueError):
                d.setSourceModelTable(bad)
        _same(_run(d), host, "after a refused table")
    # the table alone, from a side stream, without a synchronize
    other = (table * F(0.5)).astype(F)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d.setSourceModelTable(_dev(other) * 1.0)
    h.setSource(_model("table", table=other))
    _same(_run(d), _run(h), "table set alone")
    assert not np.array_equal(_run(h)[0], host[0])


@pytest.mark.gpu
def test_source_switching(cache):
    """source model -> setSourceGrid -> source model -> back to SourceRandom: each apply equals a fresh tracer's"""
    gd, p, n = _scene(3)
    grid = vr.SourceGrid(p[:200] + np.array([0.0, 0.0, 6.0], F))

    def fresh(how):
        f = _tracer(3, 0.1, rays=RAYS)
        how(f)
        return _run(f)

    model = _model("rejection")
    t = _tracer(3, 0.1, rays=RAYS)
    t.setSource(model)
    first = _run(t)
    _same(first, fresh(lambda f: f.setSource(_model("rejection"))), "model")
    t.setSource(grid)
    _same(_run(t), fresh(lambda f: f.setSource(grid)), "grid")
    t.setSource(model)
    _same(_run(t), first, "model again")
    t.setSource(None)  # vr_set_source_model(-1)
    plain = fresh(lambda f: None)
    _same(_run(t), plain, "SourceRandom")
    assert not np.array_equal(plain[0], first[0])
    # host rays and a surface source take its place as well
    t.setSource(model)
    t.setHostRays(p[:64] + np.array([0.0, 0.0, 6.0], F), np.tile(np.array([[0, 0, -1]], F), (64, 1)))
    assert _run(t)[1]["numRays"] == 64
    t.setSource(model)
    _same(_run(t), first, "model after host rays")
    t.setSurfaceSource(p[:10], n[:10], np.ones(10, F), 1.0, 1e-3)
    assert _run(t)[1]["numRays"] == 10 * RAYS
    t.clearSurfaceSource()
    _same(_run(t), plain, "SourceRandom after the surface source")


@pytest.mark.gpu
def test_one_model_object_serves_tracers_that_come_and_go(cache):
    """the registration belongs to the tracer, not to the SourceModel object: a model kept while tracers are created and
    destroyed (a new context may even get the address of the one before) works on each, also where the new context has
    registered ANOTHER text first; and the same text set again and again registers once"""
    import gc
    beam, rejection = _model("beam"), _model("rejection")
    a = _tracer(3)
    a.setSource(beam)
    want = _run(a)
    a.setSource(rejection)
    want_rejection = _run(a)
    del a
    gc.collect()
    for _ in range(3):  # (several rounds: whatever address the allocator hands back)
        b = _tracer(3)
        b.setSource(rejection)  # this context's id 0 is the OTHER text
        _same(_run(b), want_rejection, "rejection on a later tracer")
        b.setSource(beam)
        _same(_run(b), want, "beam on a later tracer")
        del b
        gc.collect()
    # two tracers side by side share the objects; fresh objects with the same text get the same id
    c, d = _tracer(3), _tracer(3)
    d.setSource(rejection)
    c.setSource(beam)
    d.setSource(beam)
    _same(_run(c), want, "side by side")
    _same(_run(d), want, "side by side, second id")
    for _ in range(5):
        c.setSource(_model("beam"))
    assert len(c._sourceIds) == 1
    assert c.registerSourceModel("again", BEAM) == c.registerSourceModel("and again", BEAM) == c._sourceIds[(BEAM, False)]
    assert c.registerSourceModel("other", LONG) != c._sourceIds[(BEAM, False)]
    _same(_run(c), want, "after registering again")


STATEFUL = """
struct VrUserModel : ModelDiffuse {
  static constexpr bool kNeedsFull = true;
  static constexpr int kStateWords = 1;
  __device__ static void init(const ModelCtx &, RayState &s, Rng &, unsigned &) { s.v[0] = 1.f; }
  template <int D>
  __device__ static Reflection surface_reflection(const ModelCtx &, RayState &, float w, const V3 &rayDir, const V3 &n,
                                                  unsigned, int, float base, Rng &rng, unsigned &t2) {
    Reflection r{base, rayDir};
    if (w - w * base > 0.f)
      r.dir = reflection_diffuse<D>(n, rng, t2);
    return r;
  }
  template <class Credit>
  __device__ static void collide(const ModelCtx &, const RayState &, float w, const V3 &, const V3 &, unsigned, int,
                                 Credit &&credit) {
    credit(0, w);
  }
};
"""


@pytest.mark.gpu
def test_refusals_leave_the_source_in_force(cache):
    import ctypes as C
    t = _tracer(3, 0.1)
    t.setSource(_model("beam"))
    good = _run(t)
    # a text that does not compile: VR_E_INVALID with the compiler's error line
    k = C.c_int32(-5)
    rc = t._L.vr_register_source_model(t._h, b"broken", BEAM.replace("vnormalize(dir);", "no_such_function(dir);").encode(),
                                       0, C.byref(k))
    assert rc == capi.VR_E_INVALID
    msg = t._L.vr_last_error(t._h).decode()
    assert "did not compile" in msg and "no_such_function" in msg and "error" in msg
    _same(_run(t), good, "after a text that does not compile")
    with pytest.raises(vr.VrError, match="kHasWeight differs"):
        t.registerSourceModel("flag", BEAM, hasWeight=True)
    # 17 parameters, an unknown id
    p17 = (C.c_float * 17)()
    assert t._L.vr_set_source_model(t._h, 0, p17, 17, None, 0, 0) == capi.VR_E_INVALID
    assert "at most 16" in t._L.vr_last_error(t._h).decode()
    _same(_run(t), good, "after 17 parameters")
    assert t._L.vr_set_source_model(t._h, 99, None, 0, None, 0, 0) == capi.VR_E_INVALID
    assert "unknown source model" in t._L.vr_last_error(t._h).decode()
    _same(_run(t), good, "after an unknown id")
    # a stateful particle model with a source model: refused at prepare, in the words the other sources get
    kind = t.registerParticleModel(STATEFUL, numData=1, numState=1)
    t.setParticleType(vr.UserModelParticle(kind, 0.1, ["flux"]))
    with pytest.raises(vr.VrError, match="SourceRandom only.*source model"):
        t.apply()
    t.setParticleType(vr.DiffuseParticle(0.1, "flux"))
    _same(_run(t), good, "after the stateful refusal")


@pytest.mark.gpu
def test_cpp_facade_source_model(tmp_path, cache):
    """tests/aux/facade_source_model.cpp: registerSourceModel + setSourceModel + apply() through the C++ façade; its flux
    checksum (the sum of the float bit patterns) is this module's for the same plane, source and seed"""
    exe = tmp_path / "facade_source_model"
    lib = os.path.join(ROOT, "viennaray_amd")
    subprocess.check_call(["g++", "-O1"] + FACADE_FLAGS + [FACADE_SRC, "-o", str(exe), "-L", lib, "-lviennaray_amd",
                                                          "-L", "/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib,
                                                          "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "facade source model ok" in out.stdout, out.stdout + out.stderr
    theirs = int([l for l in out.stdout.splitlines() if l.startswith("checksum ")][0].split()[1])
    x, y = np.meshgrid(np.arange(24, dtype=F), np.arange(24, dtype=F), indexing="ij")
    p = np.stack([x.ravel(), y.ravel(), np.zeros(576, F)], axis=1)
    t = vr.TraceDisk(3)
    t.setGeometry(p, np.tile(np.array([[0, 0, 1]], F), (576, 1)), 1.0)
    t.setRngSeed(SEED)
    t.setParticleType(vr.DiffuseParticle(0.1, "flux"))
    t.setSource(vr.SourceModel("beam", BEAM, params=[A, B], numRays=RAYS))
    t.apply()
    flux = t.getLocalData().getVectorData(0)
    assert flux.sum() > 0
    assert int(flux.view(np.uint32).astype(np.uint64).sum()) == theirs
