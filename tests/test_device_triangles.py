"""Device-resident triangle meshes in (vr_set_triangles_device, TraceTriangle.setGeometry on torch tensors).

The device way must feed the same bytes into the same kernels as the host way: everything below compares with `==` /
np.array_equal on the host path's result for the same inputs and settings, there is no tolerance anywhere.  (The sort
plane of the ray stream is the one value that may differ in its last bits — it only orders work — and is not compared.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import viennaray_amd as vr
from viennaray_amd import capi
from helpers import DATA, ROOT, trench3d, trench_mesh

PER = vr.BoundaryCondition.PERIODIC_BOUNDARY
REF = vr.BoundaryCondition.REFLECTIVE_BOUNDARY
SOURCE = vr.NormalizationType.SOURCE
INFO_KEYS = ("numRays", "totalRaysTraced", "nonGeometryHits", "geometryHits", "particleHits", "boundaryHits",
             "reflections", "raysTerminated", "warning", "error", "rngFullStates", "bvhRefits", "bvhBuilds")
FACADE_FLAGS = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include",
                "-I", os.path.join(ROOT, "include", "viennaray_amd"), "-I", os.path.join(ROOT, "include")]
FACADE_SRC = os.path.join(ROOT, "tests", "aux", "facade_device_triangles.cpp")
INGEST_MAX_BLOCKS = 1024  # vr_ingest.hip: the grid-stride cap of the ingest kernels, tiles of 256 rows


# ---------------------------------------------------------------------------------------------------------------------
# no GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_device_triangle_entry_point_is_declared_exported_and_bound():
    txt = open(os.path.join(ROOT, "include", "viennaray_amd.h")).read()
    L = vr.load()
    assert "vr_set_triangles_device(" in txt
    assert hasattr(L, "vr_set_triangles_device")
    assert "vr_set_triangles_device" in capi.SIGNATURES
    assert len(capi.SIGNATURES["vr_set_triangles_device"][1]) == 8
    assert callable(getattr(vr.TraceTriangle, "_setGeometryDevice", None))


def test_cpp_facade_declares_set_geometry_device_on_trace_triangle():
    """TraceTriangle<T, D>::setGeometryDevice: tests/aux/facade_device_triangles.cpp compiles"""
    hdr = open(os.path.join(ROOT, "include", "viennaray_amd", "viennaray.hpp")).read()
    assert "void setGeometryDevice(const float *dVerts, size_t nverts, const unsigned *dTris, size_t ntris" in hdr
    p = subprocess.run(["g++", "-fsyntax-only"] + FACADE_FLAGS + [FACADE_SRC], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]


def test_line_geometry_docstring_says_that_it_is_host_only():
    assert "out of scope" in vr.TraceTriangle.setLineGeometry.__doc__


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def _torch():
    import torch
    return torch


def grid_mesh(nt, width=16, ripple=0.3, gd=1.0):
    """the first nt triangles of a grid of `width` cells per row (two triangles per cell, normals towards +z), the
    vertices rippled by `ripple` grid cells"""
    cells = (nt + 1) // 2
    rows = (cells + width - 1) // width
    i, j = np.meshgrid(np.arange(rows + 1), np.arange(width + 1), indexing="ij")
    z = ripple * gd * np.sin(0.9 * j) * np.cos(0.7 * i)
    v = np.stack([j.ravel() * gd, i.ravel() * gd, z.ravel()], axis=1).astype(np.float32)
    c = np.arange(cells)
    a = (c // width) * (width + 1) + c % width
    b, d, e = a + 1, a + width + 1, a + width + 2
    t = np.empty((2 * cells, 3), dtype=np.uint32)
    t[0::2] = np.stack([a, b, d], 1)
    t[1::2] = np.stack([b, e, d], 1)
    return gd, v, np.ascontiguousarray(t[:nt])


def line_mesh():
    gd, nodes, lines = vr.io.read_line_mesh(os.path.join(DATA, "lineMesh.dat"))
    v, t, _ = vr.io.lines_to_triangles(nodes, lines, gd)
    return gd, v, t


def _tensors(v, t):
    torch = _torch()
    return (torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda(),
            torch.from_numpy(np.ascontiguousarray(t).astype(np.uint32).view(np.int32)).cuda())


def _configure(t, D, sticking, bc, rays, particle=None, direction=None):
    t.setBoundaryConditions([bc] * D)
    if direction is not None:
        t.setSourceDirection(direction)
    t.setParticleType(particle or vr.DiffuseParticle(sticking, "flux"))
    t.setNumberOfRaysFixed(rays)
    t.setUseRandomSeeds(False)
    t.setRngSeed(4711)


def _observe(t, mesh_bits=True, bvh=True):
    i = t.getRayTraceInfo()
    ld = t.getLocalData()
    flux = [ld.getVectorData(k).copy() for k in range(t.numData())]
    obs = dict(bbox=t.getBoundingBox().copy(), sourceArea=t.getSourceArea(), mode=t.traceMode(),
               info={k: int(getattr(i, k)) for k in INFO_KEYS}, flux=flux,
               normalized=[t.normalizeFlux(f, SOURCE) for f in flux], bvhCheck=t.debugBvhCheck() if bvh else 0)
    if mesh_bits:
        obs["normals"], obs["areas"] = t.debugTriangleMesh()
    return obs


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_same(a, b):
    assert np.array_equal(_bits(a["bbox"]), _bits(b["bbox"])), (a["bbox"], b["bbox"])
    assert a["sourceArea"] == b["sourceArea"]
    assert a["mode"] == b["mode"]
    assert a["info"] == b["info"]
    assert len(a["flux"]) == len(b["flux"])
    for x, y in zip(a["flux"], b["flux"]):
        assert np.array_equal(_bits(x), _bits(y))
    for x, y in zip(a["normalized"], b["normalized"]):  # (SOURCE divides by the areas; bits: a zero area gives inf / NaN on both)
        assert np.array_equal(_bits(x), _bits(y))
    if "normals" in a and "normals" in b:
        assert np.array_equal(_bits(a["normals"]), _bits(b["normals"]))
        assert np.array_equal(_bits(a["areas"]), _bits(b["areas"]))


def _assert_clean_build(obs):
    assert obs["info"]["bvhRefits"] == 0 and obs["bvhCheck"] == 0


def _host_run(D, gd, v, t, sticking, bc, rays, **kw):
    tr = vr.TraceTriangle(D)
    tr.setGeometry(v, t, gd)
    _configure(tr, D, sticking, bc, rays, **kw)
    tr.apply()
    return tr


def _device_run(D, gd, v, t, sticking, bc, rays, **kw):
    tr = vr.TraceTriangle(D)
    tr.setGeometry(*_tensors(v, t), gd)
    _configure(tr, D, sticking, bc, rays, **kw)
    tr.apply()
    return tr


@pytest.fixture(scope="module")
def trench_reference():
    """one host-geometry run of trenchMesh.dat (sticking 0.1, periodic), shared by the tests that compare against it"""
    gd, v, t = trench_mesh()
    rays = 200_000
    tr = _host_run(3, gd, v, t, 0.1, PER, rays)
    return dict(scene=(gd, v, t, rays), obs=_observe(tr))


@pytest.mark.gpu
@pytest.mark.parametrize("sticking", [1.0, 0.1])
@pytest.mark.parametrize("bc", [REF, PER])
def test_trench_mesh_tensors_equal_host_arrays(sticking, bc):
    """two fresh contexts, the same seed: host arrays in one, device tensors in the other — box, source area, normals,
    areas, trace mode, every counter, every raw and SOURCE-normalised flux bit are the same"""
    gd, v, t = trench_mesh()
    a = _observe(_host_run(3, gd, v, t, sticking, bc, 200_000))
    b = _observe(_device_run(3, gd, v, t, sticking, bc, 200_000))
    _assert_same(a, b)
    _assert_clean_build(b)
    assert a["info"]["error"] == 0 and a["info"]["numRays"] == 200_000 and a["flux"][0].any()


@pytest.mark.gpu
def test_line_mesh_strips_as_tensors_use_the_even_odd_area_rule():
    """D == 2: lineMesh.dat through io.lines_to_triangles; the area of a strip triangle is half the length of its edge
    v1 - v0 (even) or v2 - v0 (odd), rayGeometryTriangle.hpp:62-75"""
    gd, v, t = line_mesh()
    for sticking in (1.0, 0.1):
        a = _observe(_host_run(2, gd, v, t, sticking, REF, 50_000))
        b = _observe(_device_run(2, gd, v, t, sticking, REF, 50_000))
        _assert_same(a, b)
        _assert_clean_build(b)
    e = np.where((np.arange(t.shape[0]) % 2 == 0)[:, None], v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
    want = 0.5 * np.linalg.norm(e.astype(np.float64), axis=1)
    assert np.allclose(b["areas"], want, rtol=1e-6) and a["flux"][0].any()


@pytest.mark.gpu
@pytest.mark.parametrize("nt", [1, 255, 256, 257, 513])
def test_grid_meshes_on_the_tile_edges(nt):
    gd, v, t = grid_mesh(nt)
    for sticking in (1.0, 0.1):
        a = _observe(_host_run(3, gd, v, t, sticking, REF, 4000))
        b = _observe(_device_run(3, gd, v, t, sticking, REF, 4000))
        _assert_same(a, b)
        _assert_clean_build(b)
    assert a["info"]["geometryHits"] > 0


@pytest.mark.gpu
def test_a_mesh_just_past_the_grid_stride_limit():
    """256 x INGEST_MAX_BLOCKS + 1 triangles: the first block of the pack pass takes a second tile, of one triangle"""
    nt = 256 * INGEST_MAX_BLOCKS + 1
    gd, v, t = grid_mesh(nt, width=512)
    a = _observe(_host_run(3, gd, v, t, 0.1, PER, 200_000))
    b = _observe(_device_run(3, gd, v, t, 0.1, PER, 200_000))
    _assert_same(a, b)
    _assert_clean_build(b)
    assert a["info"]["geometryHits"] > 0


@pytest.mark.gpu
def test_bounding_box_counts_unreferenced_vertices_and_keeps_the_first_zero():
    """rayMesh.hpp:12-25: the box is over ALL nodes, referenced or not, all three columns; std::min / std::max keep the
    first of equal values, and -0 == +0, so the box ends with the sign of the first zero"""
    gd, v, t = grid_mesh(300, ripple=0.0)
    for first, second in ((0.0, -0.0), (-0.0, 0.0)):
        w = np.concatenate([v, np.array([[-7.5, 40.25, 0.0]], dtype=np.float32)])  # the outlier: no triangle uses it
        w[:, 2] = np.where(np.arange(w.shape[0]) % 2 == 0, np.float32(first), np.float32(second))
        host, dev = vr.TraceTriangle(3), vr.TraceTriangle(3)
        host.setGeometry(w, t, gd)
        dev.setGeometry(*_tensors(w, t), gd)
        for tr in (host, dev):
            _configure(tr, 3, 1.0, PER, 1000, direction=vr.TraceDirection.POS_X)  # (the z extent is not padded)
            tr.applyPrepare()
        hb, db = host.getBoundingBox(), dev.getBoundingBox()
        assert np.array_equal(_bits(hb), _bits(db)), (hb, db)
        assert hb[0, 0] == np.float32(-7.5) and np.signbit(hb[0, 2]) == np.signbit(np.float32(first))


@pytest.mark.gpu
def test_a_degenerate_triangle_gets_the_hosts_normal_and_area_bits():
    """two equal vertices: a zero cross product, which normalize3 leaves as it is, and a zero area — no NaN that the
    host does not produce"""
    gd, v, t = grid_mesh(300)
    t = t.copy()
    t[17, 1] = t[17, 0]
    t[256, 2] = t[256, 1]
    host, dev = vr.TraceTriangle(3), vr.TraceTriangle(3)
    host.setGeometry(v, t, gd)
    dev.setGeometry(*_tensors(v, t), gd)
    (hn, ha), (dn, da) = host.debugTriangleMesh(), dev.debugTriangleMesh()
    assert np.array_equal(_bits(hn), _bits(dn)) and np.array_equal(_bits(ha), _bits(da))
    assert not np.isnan(dn).any() and not np.isnan(da).any()
    assert not dn[17].any() and da[17] == 0.0 and not dn[256].any()
    for tr in (host, dev):
        _configure(tr, 3, 0.1, REF, 4000)
        tr.apply()
    _assert_same(_observe(host), _observe(dev))


@pytest.mark.gpu
def test_an_index_out_of_range_is_refused_and_names_the_triangle(trench_reference):
    torch = _torch()
    gd, v, t, rays = trench_reference["scene"]
    tr = vr.TraceTriangle(3)
    tv, tt = _tensors(v, t)
    tr.setGeometry(tv, tt, gd)
    _configure(tr, 3, 0.1, PER, rays)
    gd2, v2, t2 = grid_mesh(513)
    tv2, _ = _tensors(v2, t2)
    nv = v2.shape[0]
    cases = []
    bad = t2.astype(np.int64)
    bad[300, 1] = nv  # the first value that is out of range
    bad[400, 0] = nv + 5  # (a later one: the lowest triangle is reported)
    cases.append((bad, 300))
    bad = t2.astype(np.int64)
    bad[5, 2] = -1  # a negative int32 reads as 0xFFFFFFFF
    cases.append((bad, 5))
    bad = t2.astype(np.int64)
    bad[512, 2] = nv  # the last triangle, in the third tile
    cases.append((bad, 512))
    for idx, where in cases:
        ti = torch.from_numpy(idx.astype(np.int32)).cuda()
        with pytest.raises(vr.VrError, match=rf"vertex index out of range \(triangle {where}\)"):
            tr.setGeometry(tv2, ti, gd2)
    # the previous geometry is still in place
    assert tr._n == t.shape[0]
    tr.apply()
    _assert_same(trench_reference["obs"], _observe(tr))
    # ... and after the two refusals of the C entry points themselves, one that comes with the scan's verdict and one
    # that comes before anything is looked at: the code, and the previous geometry's flux exactly
    L = capi.load()
    ptr = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    one_bad = t2.astype(np.int64)
    one_bad[100, 0] = nv
    ti = torch.from_numpy(one_bad.astype(np.int32)).cuda()
    refusals = [lambda: L.vr_set_triangles_device(tr._h, ptr(tv2), nv, ptr(ti), t2.shape[0], gd2, 3, None),
                lambda: L.vr_set_disks_device(tr._h, ptr(tv2), ptr(tv2), nv, 2, gd2, 0.0, 3, None)]  # ld = 2, D = 3
    for refused, said in zip(refusals, (b"vertex index out of range (triangle 100)", b"D == 2")):
        assert refused() == capi.VR_E_INVALID
        assert said in L.vr_last_error(tr._h)
        assert L.vr_num_primitives(tr._h) == t.shape[0]
        tr.setRunNumber(1)  # (every apply advances it: the reference traced run 1)
        tr.apply()
        _assert_same(trench_reference["obs"], _observe(tr))


class _ElsewhereTensor:
    """a real device tensor that says it lives on another device index (one GPU is enough to test the refusal)"""

    def __init__(self, x, index):
        self._x = x
        self.device = _torch().device("cuda", index)
        self.is_cuda = True

    def __getattr__(self, name):
        return getattr(self._x, name)


@pytest.mark.gpu
def test_tensors_that_cannot_be_handed_over_raise_value_error(trench_reference):
    torch = _torch()
    L = capi.load()
    gd, v, t, rays = trench_reference["scene"]
    tv, tt = _tensors(v, t)
    tr = vr.TraceTriangle(3)
    with pytest.raises(ValueError, match="device"):
        tr.setGeometry(tv, tt.cpu(), gd)  # a host tensor beside a device tensor
    with pytest.raises(ValueError, match="device"):
        tr.setGeometry(v, tt, gd)  # a numpy array beside a device tensor
    with pytest.raises(ValueError, match="dtype"):
        tr.setGeometry(tv.double(), tt, gd)
    with pytest.raises(ValueError, match="dtype"):
        tr.setGeometry(tv, tt.long(), gd)
    with pytest.raises(ValueError, match="shape"):
        tr.setGeometry(tv.reshape(-1), tt, gd)
    with pytest.raises(ValueError, match="shape"):
        tr.setGeometry(tv, torch.zeros(10, 2, dtype=torch.int32, device="cuda"), gd)
    wide_v = torch.zeros(v.shape[0], 4, device="cuda")
    wide_t = torch.zeros(t.shape[0], 4, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="contiguity"):
        tr.setGeometry(wide_v[:, :3], tt, gd)
    with pytest.raises(ValueError, match="contiguity"):
        tr.setGeometry(tv, wide_t[:, :3], gd)
    with pytest.raises(ValueError, match="device"):
        tr.setGeometry(_ElsewhereTensor(tv, 1), tt, gd)  # another device index
    with pytest.raises(ValueError, match="device"):
        tr.setGeometry(tv, _ElsewhereTensor(tt, 1), gd)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="device"):
            tr.setGeometry(tv.to("cuda:1"), tt.to("cuda:1"), gd)
    # ... and the C entry point's own refusals, each with its own message
    ptr = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    nv, nt = v.shape[0], t.shape[0]
    assert L.vr_set_triangles_device(tr._h, ptr(tv), nv, ptr(tt), nt, gd, 4, None) == capi.VR_E_INVALID
    assert b"bad argument" in L.vr_last_error(tr._h)
    assert L.vr_set_triangles_device(tr._h, ptr(tv), nv, ptr(tt), 1 << 27, gd, 3, None) == capi.VR_E_INVALID
    assert b"bad argument" in L.vr_last_error(tr._h)
    host_t = np.ascontiguousarray(t)
    assert L.vr_set_triangles_device(tr._h, v.ctypes.data, nv, host_t.ctypes.data, nt, gd, 3, None) == capi.VR_E_INVALID
    assert b"not device memory" in L.vr_last_error(tr._h)
    assert L.vr_set_triangles_device(tr._h, ptr(tv), nv, host_t.ctypes.data, nt, gd, 3, None) == capi.VR_E_INVALID
    assert b"not device memory" in L.vr_last_error(tr._h)
    # the context never saw a geometry: a valid call still works, and a refusal after it keeps it
    tr.setGeometry(tv, tt, gd)
    assert L.vr_set_triangles_device(tr._h, v.ctypes.data, nv, host_t.ctypes.data, nt, gd, 3, None) == capi.VR_E_INVALID
    _configure(tr, 3, 0.1, PER, rays)
    tr.apply()
    _assert_same(trench_reference["obs"], _observe(tr))


@pytest.mark.gpu
def test_an_empty_mesh_behaves_as_on_the_host_path():
    """no triangles: accepted, and apply() reports that there is no geometry — on both paths"""
    torch = _torch()
    gd, v, t = grid_mesh(4)
    errors = []
    for on_device in (False, True):
        tr = vr.TraceTriangle(3)
        if on_device:
            tr.setGeometry(torch.from_numpy(v).cuda(), torch.zeros(0, 3, dtype=torch.int32, device="cuda"), gd)
        else:
            tr.setGeometry(v, np.zeros((0, 3), np.uint32), gd)
        _configure(tr, 3, 0.1, PER, 1000)
        with pytest.raises(vr.VrError) as e:
            tr.apply()
        errors.append(str(e.value))
    assert errors[0] == errors[1] and "No geometry" in errors[0]


@pytest.mark.gpu
def test_the_library_takes_its_own_copy_at_set_time(trench_reference):
    gd, v, t, rays = trench_reference["scene"]
    tr = vr.TraceTriangle(3)
    tv, tt = _tensors(v, t)
    tr.setGeometry(tv, tt, gd)
    tv.zero_()
    tt.zero_()
    _torch().cuda.synchronize()
    _configure(tr, 3, 0.1, PER, rays)
    tr.apply()
    _assert_same(trench_reference["obs"], _observe(tr))


@pytest.mark.gpu
def test_tensors_produced_on_a_side_stream_need_no_synchronize(trench_reference):
    """both tensors are written by kernels queued on a non-default stream behind a few large matmuls; setGeometry, inside
    `with torch.cuda.stream(s)` and without any synchronize, must wait for them on the device"""
    torch = _torch()
    gd, v, t, rays = trench_reference["scene"]
    hv, ht = _tensors(v, t)
    a = torch.randn(3072, 3072, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    tr = vr.TraceTriangle(3)
    with torch.cuda.stream(s):
        m = a
        for _ in range(4):
            m = (m @ a) * 1e-3
        keep = (m[0, 0] * 0.0).nan_to_num(0.0)  # (0, but only once the matmuls are through)
        tv, tt = hv + keep, ht + keep.to(torch.int32)
        tr.setGeometry(tv, tt, gd)
    _configure(tr, 3, 0.1, PER, rays)
    tr.apply()
    _assert_same(trench_reference["obs"], _observe(tr))
    s.synchronize()


@pytest.mark.gpu
def test_flux_tensor_after_a_device_mesh_equals_the_host_chain(trench_reference):
    torch = _torch()
    gd, v, t, rays = trench_reference["scene"]
    tr = _device_run(3, gd, v, t, 0.1, PER, rays)
    raw = tr.getLocalData().getVectorData(0)
    assert np.array_equal(_bits(raw), _bits(trench_reference["obs"]["flux"][0]))
    for norm in (None, SOURCE, vr.NormalizationType.MAX):
        want = raw if norm is None else tr.normalizeFlux(raw, norm)
        got = tr.getFluxTensor(0, norm)
        assert got.device == torch.device("cuda", 0) and got.dtype == torch.float32 and tuple(got.shape) == (t.shape[0],)
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), norm
    assert np.array_equal(_bits(tr.getFluxTensor(0, SOURCE).cpu().numpy()), _bits(trench_reference["obs"]["normalized"][0]))


@pytest.mark.gpu
def test_device_material_ids_and_surface_source_on_a_device_mesh():
    """setMaterialIds with an int32 tensor (a material-dependent sticking) and setSurfaceSource with tensors, on a
    device-resident mesh: the results of the host-set run on the host mesh"""
    torch = _torch()
    gd, v, t = trench_mesh()
    nt = t.shape[0]
    ids = (np.arange(nt) % 3).astype(np.int32)
    particle = lambda: vr.DiffuseParticle(0.2, "flux", materialSticking={1: 0.6, 2: 1.0})  # noqa: E731
    host = vr.TraceTriangle(3)
    host.setGeometry(v, t, gd)
    host.setMaterialIds(ids)
    dev = vr.TraceTriangle(3)
    dev.setGeometry(*_tensors(v, t), gd)
    dev.setMaterialIds(torch.from_numpy(ids).cuda())
    for tr in (host, dev):
        _configure(tr, 3, 0.2, PER, 100_000, particle=particle())
        tr.apply()
    a, b = _observe(host), _observe(dev)
    _assert_same(a, b)
    _assert_clean_build(b)
    assert a["flux"][0].any()
    # a surface source: rays start above every 50th triangle's first vertex
    pos = np.ascontiguousarray(v[t[::50, 0]] + np.array([0, 0, 0.5 * gd], np.float32))
    nrm = np.tile(np.array([0, 0, 1], np.float32), (pos.shape[0], 1))
    wgt = np.linspace(0.5, 1.5, pos.shape[0]).astype(np.float32)
    host.setSurfaceSource(pos, nrm, wgt, 3.0, 0.01 * gd)
    dev.setSurfaceSource(torch.from_numpy(pos).cuda(), torch.from_numpy(nrm).cuda(), torch.from_numpy(wgt).cuda(), 3.0,
                         0.01 * gd)
    for tr in (host, dev):
        tr.setRunNumber(1)
        tr.apply()
    a, b = _observe(host), _observe(dev)
    _assert_same(a, b)
    assert a["flux"][0].any()


@pytest.mark.gpu
def test_switching_between_geometries_on_one_context():
    """disk device -> triangle device -> triangle host -> triangle device -> disk host on ONE context (the disk setters
    through the C ABI: the Python classes own one geometry kind each), one apply after each: every result is a fresh
    context's"""
    torch = _torch()
    L = capi.load()
    sticking, rays = 0.1, 50_000
    gdD, p, n = trench3d()
    gdT, v, t = trench_mesh()
    gdG, vG, tG = grid_mesh(513)
    tp, tn = torch.from_numpy(p).cuda(), torch.from_numpy(n).cuda()
    torch.cuda.synchronize()
    tr = vr.TraceTriangle(3)
    _configure(tr, 3, sticking, PER, rays)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731

    def fresh_disk():
        f = vr.TraceDisk(3)
        f.setGeometry(p, n, gdD)
        _configure(f, 3, sticking, PER, rays)
        f.apply()
        return f

    def apply_and_compare(fresh, mesh_bits):
        tr.setRunNumber(1)  # (every apply advances it: the fresh contexts trace run 1)
        tr.apply()
        a, b = _observe(fresh, mesh_bits), _observe(tr, mesh_bits)
        a["info"].pop("bvhBuilds"), b["info"].pop("bvhBuilds")  # (the reused context has built more scenes)
        _assert_same(a, b)
        _assert_clean_build(b)

    tr._check(L.vr_set_disks_device(tr._h, C.c_void_p(tp.data_ptr()), C.c_void_p(tn.data_ptr()), p.shape[0], 3, gdD, 0.0, 3,
                                    None))
    tr._n = p.shape[0]
    apply_and_compare(fresh_disk(), False)
    tr.setGeometry(*_tensors(v, t), gdT)
    apply_and_compare(_host_run(3, gdT, v, t, sticking, PER, rays), True)
    tr.setGeometry(vG, tG, gdG)
    apply_and_compare(_host_run(3, gdG, vG, tG, sticking, PER, rays), True)
    tr.setGeometry(*_tensors(v, t), gdT)  # (a device mesh over a host mesh)
    apply_and_compare(_host_run(3, gdT, v, t, sticking, PER, rays), True)
    tr._check(L.vr_set_disks(tr._h, fp(p), fp(n), p.shape[0], gdD, 0.0, 3))
    tr._n = p.shape[0]
    apply_and_compare(fresh_disk(), False)
    tr.setGeometry(*_tensors(vG, tG), gdG)  # (a device mesh over host disks)
    apply_and_compare(_host_run(3, gdG, vG, tG, sticking, PER, rays), True)


@pytest.mark.gpu
def test_every_kind_and_side_in_turn_on_one_context():
    """host disks -> device disks -> host triangles -> device triangles -> host disks on ONE context, an 8 x 8 plane
    patch as 64 disks and as 98 triangles, 2000 rays after each step: flux, box and primitive count are a fresh context's,
    bit for bit.  Every setter ends in the same commit: nothing of the previous kind or side may survive it."""
    torch = _torch()
    L = capi.load()
    rays = 2000
    gd, v, t = grid_mesh(98, width=7, ripple=0.0)
    p = v.copy()
    n = np.zeros_like(p)
    n[:, 2] = 1.0
    assert p.shape == (64, 3) and t.shape == (98, 3)
    tp, tn = torch.from_numpy(p).cuda(), torch.from_numpy(n).cuda()
    tv, tt = _tensors(v, t)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    ptr = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731

    def observe(tr, count):
        tr._n = count
        tr.setRunNumber(1)  # (every apply advances it)
        tr.apply()
        return dict(flux=tr.getLocalData().getVectorData(0).copy(), bbox=tr.getBoundingBox().copy(),
                    count=int(L.vr_num_primitives(tr._h)))

    def fresh(set_geometry, count):
        f = vr.TraceTriangle(3)
        _configure(f, 3, 0.1, PER, rays)
        f._check(set_geometry(f))
        return observe(f, count)

    setters = dict(
        host_disks=lambda tr: L.vr_set_disks(tr._h, fp(p), fp(n), 64, gd, 0.0, 3),
        device_disks=lambda tr: L.vr_set_disks_device(tr._h, ptr(tp), ptr(tn), 64, 3, gd, 0.0, 3, None),
        host_triangles=lambda tr: L.vr_set_triangles(tr._h, fp(v), 64, t.ctypes.data_as(C.POINTER(C.c_uint32)), 98, gd, 3),
        device_triangles=lambda tr: L.vr_set_triangles_device(tr._h, ptr(tv), 64, ptr(tt), 98, gd, 3, None))
    want = dict(disks=fresh(setters["host_disks"], 64), triangles=fresh(setters["host_triangles"], 98))
    assert want["disks"]["count"] == 64 and want["triangles"]["count"] == 98
    assert want["disks"]["flux"].any() and want["triangles"]["flux"].any()
    tr = vr.TraceTriangle(3)
    _configure(tr, 3, 0.1, PER, rays)
    for step in ("host_disks", "device_disks", "host_triangles", "device_triangles", "host_disks"):
        tr._check(setters[step](tr))
        kind = step.split("_")[1]
        got = observe(tr, want[kind]["count"])
        assert got["count"] == want[kind]["count"], step
        assert np.array_equal(_bits(got["bbox"]), _bits(want[kind]["bbox"])), step
        assert np.array_equal(_bits(got["flux"]), _bits(want[kind]["flux"])), step


@pytest.mark.gpu
def test_host_build_after_a_device_mesh_reads_the_lazy_mirror(monkeypatch):
    """VR_HOST_BUILD: the LBVH and the sort plane on the host, from verts / tris / normal3 / triAreas downloaded on
    demand (no device-built BVH to check)"""
    gd, v, t = grid_mesh(513)
    monkeypatch.setenv("VR_HOST_BUILD", "1")
    a = _observe(bvh=False, t=_host_run(3, gd, v, t, 0.1, PER, 20_000))
    b = _observe(bvh=False, t=_device_run(3, gd, v, t, 0.1, PER, 20_000))
    _assert_same(a, b)
    assert a["info"]["geometryHits"] > 0
    gd, v, t = line_mesh()
    a = _observe(bvh=False, t=_host_run(2, gd, v, t, 0.1, REF, 20_000))
    b = _observe(bvh=False, t=_device_run(2, gd, v, t, 0.1, REF, 20_000))
    _assert_same(a, b)


@pytest.mark.gpu
def test_cpp_facade_device_triangles(tmp_path):
    """tests/aux/facade_device_triangles.cpp: hipMalloc, fill, setGeometryDevice, apply — bit-equal to the
    setGeometry(TriangleMesh) façade"""
    exe = tmp_path / "facade_device_triangles"
    lib = os.path.join(ROOT, "viennaray_amd")
    subprocess.check_call(["g++", "-O1"] + FACADE_FLAGS + [FACADE_SRC, "-o", str(exe), "-L", lib, "-lviennaray_amd",
                                                          "-L", "/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib,
                                                          "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "facade device triangles ok" in out.stdout, out.stdout + out.stderr
