"""The data log of a stateful device particle model (vr_particles.hpp: kLogRows, log_data; vr_set_data_log_shape): the
reference's logData, called once per ray right after initNew (rayTraceKernel.hpp:131-133), and its per-thread DataLog
merged into Trace::getDataLog() (rayTraceKernel.hpp:345).

The oracle has no DataLog.  The expectations are rebuilt from the engine it exposes: ray i of an apply owns
mt19937_64(tea3(i, rngSeed + runNumber)); the test model's init takes output 0, E = 2 * canon_f32(output 0), and logs
log(0, (int)(E * bins / 2), 1) and log(1, (int)(E * bins / 2), E).  Every step is exact in float32 (a power-of-two scale, a
truncation), and the log is an int64 sum of q(v) = (u64)((double)v * 2^24 + 0.5) per call: device and rebuild must agree
bit for bit, whatever the grid, the batch split and the accumulation path."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import viennaray_amd as vr
from viennaray_amd import BoundaryCondition as BC, TraceDirection as TD
from oracle import pyoracle as po
from helpers import trench2d, trench3d, trench_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "viennaray_amd", "csrc")
INFO_KEYS = ("numRays", "totalRaysTraced", "nonGeometryHits", "geometryHits", "particleHits",
             "boundaryHits", "reflections", "raysTerminated")
FRAC = 24  # VR_LOG_FRAC_BITS

HOOKS = """
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
"""
# E = 2 * canon_f32(output 0); bin = (int)(E * params[0]).  params[1] chooses what is logged:
#   0  the known answer: log(0, bin, 1), log(1, bin, E)
#   1  the dropped contract: by bin & 7 a bin beyond the row, a negative value, a NaN, a value above 2^15, a row beyond
#      the shape, a negative bin — all dropped — or (6, 7) the count; log(1, bin, E) always
#   2  the overflow case: log(0, 0, 2^15), the largest value, from every ray
#   3  a second model of a particle list: log(0, bin, 2), log(1, bin, E / 2)
LOGGER = """
struct VrUserModel : ModelDiffuse {
  static constexpr bool kNeedsFull = true;
  static constexpr int kStateWords = 1;
  static constexpr int kLogRows = 2;
  __device__ static void init(const ModelCtx &, RayState &s, Rng &rng, unsigned &t2) { s.v[0] = 2.f * canon_f32(rng_next(rng, t2)); }
  template <class Log> __device__ static void log_data(const ModelCtx &m, const RayState &s, Log &&log) {
    const float E = s.v[0];
    const int bin = (int)(E * m.params[0]), what = (int)m.params[1];
    if (what == 0) {
      log(0, bin, 1.f);
      log(1, bin, E);
    } else if (what == 1) {
      switch (bin & 7) {
      case 0: log(0, 64 + bin, 1.f); break;
      case 1: log(0, bin, -1.f); break;
      case 2: log(0, bin, __int_as_float(0x7fc00000)); break;
      case 3: log(0, bin, 40000.f); break;
      case 4: log(2, bin, 1.f); break;
      case 5: log(0, -1, 1.f); break;
      default: log(0, bin, 1.f);
      }
      log(1, bin, E);
    } else if (what == 2) {
      log(0, 0, 32768.f);
    } else {
      log(0, bin, 2.f);
      log(1, bin, 0.5f * E);
    }
  }
""" + HOOKS + "};\n"
# the same model without the hook
SILENT = """
struct VrUserModel : ModelDiffuse {
  static constexpr bool kNeedsFull = true;
  static constexpr int kStateWords = 1;
  __device__ static void init(const ModelCtx &, RayState &s, Rng &rng, unsigned &t2) { s.v[0] = 2.f * canon_f32(rng_next(rng, t2)); }
""" + HOOKS + "};\n"


@pytest.fixture(scope="module")
def model_cache(tmp_path_factory):
    """one code-object cache for the module: each model is compiled once"""
    return str(tmp_path_factory.mktemp("vr_log_cache"))


def _scene(geom):
    if geom == "mesh":
        gd, v, tri = trench_mesh()
        t = vr.TraceTriangle(3)
        t.setGeometry(v, tri, gd)
        return t
    gd, p, n = {"trench3d": trench3d, "trench2d": trench2d}[geom]()
    D = 2 if geom == "trench2d" else 3
    t = vr.TraceDisk(D)
    t.setGeometry(p, n, gd)
    if D == 2:
        t.setSourceDirection(TD.POS_Y)
        t.setBoundaryConditions([BC.PERIODIC_BOUNDARY] * 2)
    return t


def _setup(geom, cache, monkeypatch, rays, seed, source=LOGGER, params=(32.0, 0.0), sticking=0.3, name="logger"):
    monkeypatch.setenv("VR_CACHE_DIR", cache)
    t = _scene(geom)
    t.setNumberOfRaysFixed(rays)
    t.setRngSeed(seed)
    k = t.registerParticleModel(source, numData=1, name=name, numState=1)
    t.setParticleType(vr.UserModelParticle(k, sticking, ["flux"], params=list(params)))
    return t, k


def _info(t):
    i = t.getRayTraceInfo()
    return {k: int(getattr(i, k)) for k in INFO_KEYS}


@functools.lru_cache(maxsize=None)
def _energies(first, count, kernel_seed):
    """E of the rays [first, first + count): 2 * canon_f32(output 0 of mt19937_64(tea3(i, kernel_seed))), float32"""
    raw = np.array([po.mt64_outputs(po.tea3(i, kernel_seed), 1)[0] for i in range(first, first + count)], dtype=np.uint64)
    return (np.float32(2.0) * po.uniform_float(raw)).astype(np.float32)


def _q(v):
    """(u64)((double)v * 2^24 + 0.5) of float32 values"""
    return np.floor(np.asarray(v, dtype=np.float32).astype(np.float64) * 2.0 ** FRAC + 0.5).astype(np.int64)


def _rebuild(E, scale, rows=(64, 64), count=1.0, energy=1.0):
    """the int64 log of log(0, bin, count), log(1, bin, energy * E) per ray, rows concatenated"""
    b = (E * np.float32(scale)).astype(np.int32)
    assert b.min() >= 0 and b.max() < min(rows)
    out = np.zeros(sum(rows), dtype=np.int64)
    np.add.at(out, b, _q(np.full(E.size, count, dtype=np.float32)))
    np.add.at(out, rows[0] + b, _q(np.float32(energy) * E))
    return out


def _to_float(acc):
    return (acc.astype(np.float64) * 2.0 ** -FRAC).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("geom,primary,plain", [("trench3d", False, False), ("trench3d", True, False),
                                                ("trench2d", False, False), ("trench2d", True, False),
                                                ("mesh", False, False), ("mesh", True, False),
                                                ("trench3d", False, True)])
def test_known_answer_bit_for_bit(geom, primary, plain, model_cache, monkeypatch):
    """200 000 rays in batches of 32 768 (seven generator launches of 128 blocks: every entry is flushed many times):
    the int64 log equals the rebuild, the float view is its conversion, row 0 counts every ray once.  `plain`: the same
    through the direct global atomics (VR_LOG_PLAIN_ATOMICS)."""
    monkeypatch.setenv("VR_BATCH_RAYS", "32768")
    if plain:
        monkeypatch.setenv("VR_LOG_PLAIN_ATOMICS", "1")
    nr, seed = 200_000, 4711
    t, _ = _setup(geom, model_cache, monkeypatch, nr, seed)
    if primary:
        t.setPrimaryDirection([0.2, -1.0, 0.0] if geom == "trench2d" else [0.2, 0.1, -1.0])
    t.setDataLogShape([64, 64])
    t.setRunNumber(3)
    t.apply()
    want = _rebuild(_energies(0, nr, seed + 3), 32.0)
    got = t.dataLogAccumulators()
    assert got.dtype == np.int64 and (got == want).all()
    rows = t.getDataLog()
    assert len(rows) == 2 and rows[0].dtype == np.float32
    assert (np.concatenate(rows) == _to_float(want)).all()
    assert rows[0].sum(dtype=np.float64) == nr and t.getDataLogDropped() == 0
    assert _info(t)["numRays"] == nr


@pytest.mark.gpu
@pytest.mark.parametrize("geom", ["trench3d", "trench2d"])
def test_nothing_else_moves(geom, model_cache, monkeypatch):
    """The hook draws nothing: flux and every TraceInfo counter of a run with the hook and a shape are bit-equal to the
    same model without the hook."""
    nr, seed = 150_000, 99
    t, _ = _setup(geom, model_cache, monkeypatch, nr, seed)
    t.setDataLogShape([64, 64])
    t.apply()
    f_log, i_log = t.getLocalData().getVectorData(0).copy(), _info(t)
    assert t.getDataLog()[0].sum(dtype=np.float64) == nr
    s, _ = _setup(geom, model_cache, monkeypatch, nr, seed, source=SILENT, name="silent")
    s.apply()
    assert _info(s) == i_log and (s.getLocalData().getVectorData(0) == f_log).all()
    assert i_log["geometryHits"] > 0


@pytest.mark.gpu
def test_grid_and_shard_independence(model_cache, monkeypatch):
    """Two halves of the ray range add up to the full run's log; vr_apply_sharded with one rank gives it too; a repeated
    run gives identical bits."""
    nr, seed = 120_001, 31
    t, _ = _setup("trench3d", model_cache, monkeypatch, nr, seed)
    t.setDataLogShape([64, 64])

    def run(first=0, count=0, sharded=False):
        t.setRunNumber(1)
        t.setRayRange(first, count)
        if sharded:
            calls = []
            cb = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)(lambda u, p, n, s: calls.append(n) or 0)
            t.applySharded(0, 1, cb)
        else:
            t.apply()
        return t.dataLogAccumulators().copy(), t.getDataLogDropped()
    full, d0 = run()
    again, _ = run()
    lo, d1 = run(0, nr // 2)
    hi, d2 = run(nr // 2, nr - nr // 2)
    sh, _ = run(sharded=True)
    assert (full == again).all() and (full == sh).all()
    assert (lo + hi == full).all() and not (lo == hi).all() and d0 == d1 == d2 == 0
    assert (full == _rebuild(_energies(0, nr, seed + 1), 32.0)).all()
    assert (lo == _rebuild(_energies(0, nr // 2, seed + 1), 32.0)).all()


@pytest.mark.gpu
def test_large_log_takes_the_direct_path(model_cache, monkeypatch):
    """2 x 4096 entries are beyond the generator's LDS copy (VR_LOG_LDS_ENTRIES = 2048): the direct global atomics give
    the rebuild's bits."""
    nr, seed = 150_000, 8
    t, _ = _setup("trench3d", model_cache, monkeypatch, nr, seed, params=(2048.0, 0.0))
    t.setDataLogShape([4096, 4096])
    t.apply()
    want = _rebuild(_energies(0, nr, seed + 1), 2048.0, rows=(4096, 4096))
    assert (t.dataLogAccumulators() == want).all() and t.getDataLogDropped() == 0
    assert np.count_nonzero(want[:4096]) > 4000


@pytest.mark.gpu
def test_dropped_calls_are_left_out_and_counted(model_cache, monkeypatch):
    """By (bin & 7) a ray logs its count to a bin beyond the row, with a negative value, a NaN, a value above 2^15, to a
    row beyond the shape or to a negative bin: all dropped and counted, the other entries exact."""
    nr, seed = 100_000, 77
    t, _ = _setup("trench3d", model_cache, monkeypatch, nr, seed, params=(32.0, 1.0))
    t.setDataLogShape([64, 64])
    t.apply()
    E = _energies(0, nr, seed + 1)
    b = (E * np.float32(32.0)).astype(np.int32)
    keep = (b & 7) >= 6
    want = np.zeros(128, dtype=np.int64)
    np.add.at(want, b[keep], 1 << FRAC)
    np.add.at(want, 64 + b, _q(E))
    assert 0 < keep.sum() < nr
    assert (t.dataLogAccumulators() == want).all()
    assert t.getDataLogDropped() == int((~keep).sum())


@pytest.mark.gpu
def test_overflow_is_detected(model_cache, monkeypatch):
    """Every ray adds the largest value, 2^15 = 2^39 fixed-point units, to ONE entry: rays * 2^15 * 2^24 reaches 2^63 at
    rays = 2^63 / 2^39 = 2^24 = 16 777 216 exactly.  2^24 - 1 rays give 2^63 - 2^39, the largest sum a single rank
    holds, bit for bit; 2^24 rays leave the range: the apply fails with "data log overflow", TraceInfo.error = 1, and
    returns no log."""
    t, _ = _setup("trench2d", model_cache, monkeypatch, (1 << 24) - 1, 5, params=(32.0, 2.0), sticking=1.0)
    t.setDataLogShape([64, 64])
    t.apply()
    acc = t.dataLogAccumulators()
    assert int(acc[0]) == (1 << 63) - (1 << 39) and not acc[1:].any()
    assert t.getDataLog()[0][0] == np.float32(((1 << 24) - 1) * 32768.0)
    assert int(t.getRayTraceInfo().error) == 0
    t.setNumberOfRaysFixed(1 << 24)
    with pytest.raises(vr.VrError, match="data log overflow"):
        t.apply()
    assert int(t.getRayTraceInfo().error) == 1
    with pytest.raises(vr.VrError, match="no result"):
        t.getDataLog()
    with pytest.raises(vr.VrError, match="no result"):
        t.dataLogAccumulators()
    # two ranks: each may hold half as much
    t.setWorldSize(2)
    t.setNumberOfRaysFixed(1 << 23)
    with pytest.raises(vr.VrError, match="data log overflow"):
        t.apply()
    t.setNumberOfRaysFixed((1 << 23) - 1)
    t.apply()
    assert int(t.dataLogAccumulators()[0]) == (1 << 62) - (1 << 39)


@pytest.mark.gpu
def test_shapes_that_are_refused(model_cache, monkeypatch):
    """A shape with a model that has no hook, a shape with fewer rows than kLogRows and a shape beyond 16 rows / 65 536
    entries are refused with a message; clearing the shape traces as before."""
    t, k = _setup("trench3d", model_cache, monkeypatch, 10_000, 1)
    with pytest.raises(vr.VrError, match="at most 16 rows"):
        t.setDataLogShape([4] * 17)
    with pytest.raises(vr.VrError, match="at most 65536 entries"):
        t.setDataLogShape([32768, 32768, 1])
    t.setDataLogShape([32768, 32768])
    t.setDataLogShape([64])
    with pytest.raises(vr.VrError, match="too few rows"):
        t.apply()
    t.setDataLogShape([64, 64])
    t.setParticleType(vr.DiffuseParticle(0.3, "flux"))
    with pytest.raises(vr.VrError, match="log_data hook"):
        t.apply()
    s = t.registerParticleModel(SILENT, numData=1, name="silent", numState=1)
    t.setParticleType(vr.UserModelParticle(s, 0.3, ["flux"]))
    with pytest.raises(vr.VrError, match="log_data hook"):
        t.apply()
    t.setDataLogShape([])
    t.apply()
    with pytest.raises(vr.VrError, match="no result"):
        t.getDataLogDropped()
    t.setParticleType(vr.UserModelParticle(k, 0.3, ["flux"], params=[32.0, 0.0]))
    t.apply()                                            # (a hook without a shape: nothing is logged)
    assert _info(t)["numRays"] == 10_000


@pytest.mark.gpu
def test_particle_list_shares_one_log(model_cache, monkeypatch):
    """Two stateful models with hooks in one setParticleTypes: the one log holds the sum of their individual logs."""
    nr, seed = 80_000, 12
    t, ka = _setup("trench3d", model_cache, monkeypatch, nr, seed)
    kb = t.registerParticleModel(LOGGER, numData=1, name="partner", numState=1)
    assert ka != kb
    a = vr.UserModelParticle(ka, 0.3, ["a"], params=[32.0, 0.0])
    b = vr.UserModelParticle(kb, 0.6, ["b"], params=[32.0, 3.0])
    t.setDataLogShape([64, 64])

    def run(particles):
        t.setParticleTypes(particles)
        t.setRunNumber(1)
        t.apply()
        return t.dataLogAccumulators().copy()
    la, lb, both = run([a]), run([b]), run([a, b])
    E = _energies(0, nr, seed + 1)
    assert (la == _rebuild(E, 32.0)).all()
    assert (lb == _rebuild(E, 32.0, count=2.0, energy=0.5)).all()
    assert (both == la + lb).all() and t.getDataLogDropped() == 0


# ---------------------------------------------------------------------------------------------------------------------
def test_python_and_c_interfaces_name_the_data_log():
    """the entry points exist on the loaded library, in its ctypes table and on the Python Trace (no device needed)"""
    L = vr.load()
    for name in ("vr_set_data_log_shape", "vr_get_data_log", "vr_get_data_log_dropped", "vr_data_log_accumulators"):
        assert hasattr(L, name) and name in vr.capi.SIGNATURES
    for name in ("setDataLogShape", "getDataLog", "getDataLogDropped", "dataLogAccumulators"):
        assert callable(getattr(vr.Trace, name))
    header = open(os.path.join(ROOT, "include", "viennaray_amd.h")).read()
    assert "#define VR_LOG_FRAC_BITS 24" in header


def _compile_module(tmp_path, model, num_state):
    """the translation unit vr_register_particle_model writes, checked for gfx950 (no device needed)"""
    (tmp_path / "model.hpp").write_text(model)
    tu = tmp_path / "module.hip"
    tu.write_text(f"#define VR_USER_MODULE 1\n#define VR_USER_NUM_DATA 1\n#define VR_USER_NUM_STATE {num_state}\n"
                  f"#define VR_USER_MODEL_FILE \"{tmp_path / 'model.hpp'}\"\n#include <cstddef>\n"
                  f"#include \"{CSRC}/vr_trace.hip\"\n")
    hipcc = os.environ.get("VR_HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "--genco", "--offload-arch=gfx950", "-O0", "-std=c++17", "-fsyntax-only", "-I", CSRC,
                        str(tu), "-o", str(tmp_path / "module.hsaco")], capture_output=True, text=True)
    return r.returncode, r.stdout + r.stderr


def test_log_rows_are_checked_at_compile_time(tmp_path):
    """kLogRows is 0 .. 16 and needs a stateful model: the module's static_asserts say so; the test models compile."""
    rc, out = _compile_module(tmp_path, "struct VrUserModel : ModelDiffuse {\n  static constexpr int kLogRows = 1;\n};\n", 0)
    assert rc != 0 and "it needs a stateful model (kStateWords > 0)" in out
    rc, out = _compile_module(tmp_path, LOGGER.replace("kLogRows = 2", "kLogRows = 17"), 1)
    assert rc != 0 and "0 .. 16 rows of the data log" in out
    rc, out = _compile_module(tmp_path, LOGGER, 1)
    assert rc == 0, out
    rc, out = _compile_module(tmp_path, SILENT, 1)
    assert rc == 0, out


def test_cpp_facade_data_log_compiles():
    """tests/aux/facade_data_log.cpp: DataLog, Trace::getDataLog() and AbstractParticle::logData in the reference's
    spelling"""
    p = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include", "viennaray_amd"),
                        "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "aux", "facade_data_log.cpp")],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]


@pytest.mark.gpu
def test_cpp_facade_data_log_accumulates_over_applies(tmp_path, model_cache, monkeypatch):
    """the program sizes getDataLog().data and applies twice: the second apply's log is added to the first; an empty log
    stays empty; a particle without a hook leaves the log alone"""
    monkeypatch.setenv("VR_CACHE_DIR", model_cache)
    exe = tmp_path / "facade_data_log"
    lib = os.path.join(ROOT, "viennaray_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include", "viennaray_amd"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "aux", "facade_data_log.cpp"),
                           "-o", str(exe), "-L", lib, "-lviennaray_amd", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "facade data log ok" in out.stdout, out.stdout + out.stderr
