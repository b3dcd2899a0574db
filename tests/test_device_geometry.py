"""Device-resident disk geometry in (vr_set_disks_device, TraceDisk.setGeometry on torch tensors) and device-resident flux
out (vr_get_flux_device, Trace.getFluxTensor).

The device way must feed the same bytes into the same kernels as the host way: everything below compares with `==` /
np.array_equal, there is no tolerance anywhere.  (The sort plane of the ray stream is the one value that may differ in
its last bits — it only orders work — and is not compared.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import viennaray_amd as vr
from viennaray_amd import capi
from helpers import ROOT, trench2d, trench3d, sphere3d

PER = vr.BoundaryCondition.PERIODIC_BOUNDARY
REF = vr.BoundaryCondition.REFLECTIVE_BOUNDARY
INFO_KEYS = ("numRays", "totalRaysTraced", "nonGeometryHits", "geometryHits", "particleHits", "boundaryHits",
             "reflections", "raysTerminated", "warning", "error", "rngFullStates", "bvhRefits", "bvhBuilds")
FACADE_FLAGS = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include",
                "-I", os.path.join(ROOT, "include", "viennaray_amd"), "-I", os.path.join(ROOT, "include")]
FACADE_SRC = os.path.join(ROOT, "tests", "aux", "facade_device_geometry.cpp")


# ---------------------------------------------------------------------------------------------------------------------
# no GPU
# ---------------------------------------------------------------------------------------------------------------------
def test_device_entry_points_are_declared_exported_and_bound():
    txt = open(os.path.join(ROOT, "include", "viennaray_amd.h")).read()
    L = vr.load()
    for name in ("vr_set_disks_device", "vr_get_flux_device"):
        assert name + "(" in txt, name
        assert hasattr(L, name), name
        assert name in capi.SIGNATURES, name
    assert "VR_NORM_NONE" in txt and capi.VR_NORM_NONE == -1
    assert callable(getattr(vr.TraceDisk, "getFluxTensor", None))
    assert callable(getattr(vr.TraceTriangle, "getFluxTensor", None))


def test_cpp_facade_declares_the_device_entry_points():
    """TraceDisk<T, D>::setGeometryDevice and Trace<T, D>::getFluxDevice: tests/aux/facade_device_geometry.cpp compiles"""
    hdr = open(os.path.join(ROOT, "include", "viennaray_amd", "viennaray.hpp")).read()
    assert "void setGeometryDevice(const float *dPoints, const float *dNormals, size_t n, unsigned ld" in hdr
    assert "bool getFluxDevice(float *dOut, int dataIdx, NormalizationType norm, int numNeighbors" in hdr
    p = subprocess.run(["g++", "-fsyntax-only"] + FACADE_FLAGS + [FACADE_SRC], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]


def test_trace_module_does_not_import_torch():
    src = open(os.path.join(ROOT, "viennaray_amd", "trace.py")).read()
    for line in src.splitlines():
        assert not line.startswith(("import torch", "from torch")), line  # (only inside the two methods that need it)


class _StandInDevice:
    def __init__(self, kind, index):
        self.type, self.index = kind, index

    def __str__(self):
        return f"{self.type}:{self.index}"


class _StandInTensor:
    """what trace.py looks at in a torch tensor, with no torch and no device behind it"""

    def __init__(self, shape, dtype="torch.float32", index=0, contiguous=True, kind="cuda"):
        self.shape, self.dtype, self.device, self.is_cuda = tuple(shape), dtype, _StandInDevice(kind, index), kind == "cuda"
        self._contiguous = contiguous

    def data_ptr(self):
        return 0x1000

    def is_contiguous(self):
        return self._contiguous

    def stride(self):
        return tuple(int(np.prod(self.shape[k + 1:])) + (0 if self._contiguous else 1) for k in range(len(self.shape)))

    def __len__(self):
        return self.shape[0]


class _RecordingLibrary:
    """stands in for the C ABI behind a TraceDisk that was never created: records the one call that gets through"""

    def __init__(self):
        self.calls = []

    def vr_set_disks_device(self, *args):
        self.calls.append(args)
        return capi.VR_OK


def _disk_tracer_without_context(D):
    t = vr.TraceDisk.__new__(vr.TraceDisk)  # (no vr_create: no device is needed to be refused)
    t.D, t._device, t._h, t._L = D, 0, None, _RecordingLibrary()
    t._torch_stream = lambda: 0
    return t


_GOOD = dict(shape=(8, 3))
# (what is wrong with the tensor, the category word of the refusal)
DISK_TENSOR_REFUSALS = [
    (dict(shape=(8, 3), index=1), "device"),            # the wrong device index
    (dict(shape=(8, 3), kind="xpu"), "device"),         # a device type that cannot be handed over: not through the host
    (dict(shape=(8, 3), dtype="torch.float64"), "dtype"),
    (dict(shape=(24,)), "shape"),                       # 1-D
    (dict(shape=(8, 4)), "shape"),                      # 4 columns
    (dict(shape=(8, 2)), "shape"),                      # 2 columns on a 3-D tracer
    (dict(shape=(8, 3), contiguous=False), "contiguity"),
    (dict(shape=(7, 3)), "shape"),                      # points and normals differ
]


@pytest.mark.parametrize("defect,word,which", [(d, w, k) for d, w in DISK_TENSOR_REFUSALS for k in ("points", "normals", "both")
                                               if not (k == "both" and d["shape"] == (7, 3))])  # (the same shape twice)
def test_disk_tensors_that_cannot_be_handed_over_are_refused_without_a_device(defect, word, which):
    """every refusal of TraceDisk.setGeometry on tensors, by its category word, for a defect in either argument or in
    both; nothing reaches the C ABI"""
    t = _disk_tracer_without_context(3)
    p = _StandInTensor(**(defect if which != "normals" else _GOOD))
    n = _StandInTensor(**(defect if which != "points" else _GOOD))
    with pytest.raises(ValueError, match=rf"^setGeometry: {word}: "):
        t.setGeometry(p, n, 1.0)
    assert t._L.calls == []


@pytest.mark.parametrize("host_side", ["points", "normals"])
def test_one_disk_argument_on_the_host_is_refused_without_a_device(host_side):
    t = _disk_tracer_without_context(3)
    host, dev = np.zeros((8, 3), np.float32), _StandInTensor(**_GOOD)
    with pytest.raises(ValueError, match=r"^setGeometry: device: "):
        t.setGeometry(*((host, dev) if host_side == "points" else (dev, host)), 1.0)
    assert t._L.calls == []


@pytest.mark.parametrize("D,cols", [(3, 3), (2, 3), (2, 2)])
def test_disk_tensors_that_can_be_handed_over_reach_the_entry_point(D, cols):
    """(the control of the refusals above: the stand-in is accepted where a tensor would be)"""
    t = _disk_tracer_without_context(D)
    t.setGeometry(_StandInTensor((8, cols)), _StandInTensor((8, cols)), 0.5, 0.25)
    (call,) = t._L.calls
    assert [a.value if hasattr(a, "value") else a for a in call[1:]] == [0x1000, 0x1000, 8, cols, 0.5, 0.25, D, None]
    assert t._n == 8


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def _torch():
    import torch
    return torch


def _plane(n, ripple=0.0, width=32, gd=1.0):
    """the first n points of a `width`-wide unit grid, z = ripple * gd * sin * cos, normals +z"""
    i = np.arange(n)
    x, y = (i % width).astype(np.float64), (i // width).astype(np.float64)
    z = ripple * gd * np.sin(0.9 * x) * np.cos(0.7 * y)
    pts = np.stack([x * gd, y * gd, z], axis=1).astype(np.float32)
    nrm = np.zeros_like(pts)
    nrm[:, 2] = 1.0
    return gd, pts, nrm


def _scene(name):
    """(D, gridDelta, points, normals, columns handed over, rays)"""
    if name == "trench3d":
        gd, p, n = trench3d()
        return 3, gd, p, n, 3, 100_000
    if name == "trench2d_ld3":
        gd, p, n = trench2d()
        return 2, gd, p, n, 3, 50_000
    if name == "trench2d_ld2":
        gd, p, n = trench2d()
        return 2, gd, p, n, 2, 50_000
    if name == "sphere3d":
        gd, p, n = sphere3d()
        return 3, gd, p, n, 3, 100_000
    if name == "plane16":
        gd, p, n = _plane(256, 0.0, width=16)
        return 3, gd, p, n, 3, 50_000
    if name == "ripple16":
        gd, p, n = _plane(256, 0.5, width=16)
        return 3, gd, p, n, 3, 50_000
    assert name.startswith("plane_n")
    gd, p, n = _plane(int(name[7:]), 0.0)
    return 3, gd, p, n, 3, 20_000


SCENES = ["trench3d", "trench2d_ld3", "trench2d_ld2", "sphere3d", "plane16", "ripple16", "plane_n1", "plane_n63",
          "plane_n65", "plane_n1025"]


def _tensors(p, n, ld):
    torch = _torch()
    return (torch.from_numpy(np.ascontiguousarray(p[:, :ld])).cuda(), torch.from_numpy(np.ascontiguousarray(n[:, :ld])).cuda())


def _configure(t, D, sticking, bc, direction, rays, particle=None):
    t.setBoundaryConditions([bc] * D)
    if direction is not None:
        t.setSourceDirection(direction)
    t.setParticleType(particle or vr.DiffuseParticle(sticking, "flux"))
    t.setNumberOfRaysFixed(rays)
    t.setUseRandomSeeds(False)
    t.setRngSeed(4711)


def _observe(t):
    i = t.getRayTraceInfo()
    ld = t.getLocalData()
    return dict(bbox=t.getBoundingBox().copy(), sourceArea=t.getSourceArea(), diskRadius=t.getDiskRadius(),
                areas=t.getDiskAreas(), neighbors=t.getNeighborCounts(), mode=t.traceMode(),
                info={k: int(getattr(i, k)) for k in INFO_KEYS}, flux=[ld.getVectorData(k).copy() for k in range(t.numData())])


def _assert_same(a, b):
    assert np.array_equal(a["bbox"].view(np.uint32), b["bbox"].view(np.uint32)), (a["bbox"], b["bbox"])
    assert a["sourceArea"] == b["sourceArea"] and a["diskRadius"] == b["diskRadius"]
    assert np.array_equal(a["areas"].view(np.uint32), b["areas"].view(np.uint32))  # (bits: a one-disk scene's area is NaN on both)
    assert np.array_equal(a["neighbors"], b["neighbors"])
    assert a["mode"] == b["mode"]
    assert a["info"] == b["info"]
    assert len(a["flux"]) == len(b["flux"])
    for x, y in zip(a["flux"], b["flux"]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def _host_run(D, gd, p, n, ld, sticking, bc, direction, rays, particle=None):
    t = vr.TraceDisk(D)
    t.setGeometry(p[:, :ld], n[:, :ld], gd)
    _configure(t, D, sticking, bc, direction, rays, particle)
    t.apply()
    return t


def _device_run(D, gd, p, n, ld, sticking, bc, direction, rays, particle=None):
    t = vr.TraceDisk(D)
    tp, tn = _tensors(p, n, ld)
    t.setGeometry(tp, tn, gd)
    _configure(t, D, sticking, bc, direction, rays, particle)
    t.apply()
    return t


@pytest.fixture(scope="module")
def trench_reference():
    """one host-geometry run of the 3-D trench (sticking 0.1, periodic), shared by the tests that compare against it"""
    D, gd, p, n, ld, rays = _scene("trench3d")
    t = _host_run(D, gd, p, n, ld, 0.1, PER, None, rays)
    return dict(scene=(D, gd, p, n, ld, rays), obs=_observe(t))


@pytest.mark.gpu
@pytest.mark.parametrize("scene", SCENES)
def test_tensor_geometry_equals_host_geometry(scene):
    """two fresh contexts, the same seed: host arrays in one, device tensors in the other — box, source area, radius,
    disk areas, neighbourhoods, trace mode, every counter and every flux bit are the same; the source direction is set
    after the geometry, so the sort-plane histogram runs on the axis of each direction"""
    D, gd, p, n, ld, rays = _scene(scene)
    dirs = (vr.TraceDirection.POS_Y, vr.TraceDirection.NEG_Y) if D == 2 else (vr.TraceDirection.POS_Z, vr.TraceDirection.NEG_Z)
    for sticking in (1.0, 0.1):
        for bc in (PER, REF):
            for direction in dirs:
                a = _observe(_host_run(D, gd, p, n, ld, sticking, bc, direction, rays))
                b = _observe(_device_run(D, gd, p, n, ld, sticking, bc, direction, rays))
                _assert_same(a, b)
                assert a["info"]["error"] == 0 and a["info"]["numRays"] == rays


@pytest.mark.gpu
def test_bounding_box_keeps_the_first_zero_like_the_host():
    """std::min / std::max keep the first of equal values, and -0 == +0: the host's box ends with the sign of the first
    row's zero.  The device reduction gives the same bits, whichever zero comes first."""
    gd, p, n = _plane(300, 0.0)
    for first, second in ((0.0, -0.0), (-0.0, 0.0)):
        q = p.copy()
        q[:, 2] = np.where(np.arange(300) % 2 == 0, np.float32(first), np.float32(second))  # z: zeros of both signs
        host, dev = vr.TraceDisk(3), vr.TraceDisk(3)
        host.setGeometry(q, n, gd)
        dev.setGeometry(*_tensors(q, n, 3), gd)
        for t in (host, dev):
            _configure(t, 3, 1.0, PER, vr.TraceDirection.POS_X, 1000)  # (the z extent is not padded: the box shows the zeros)
            t.applyPrepare()
        assert np.array_equal(host.getBoundingBox().view(np.uint32), dev.getBoundingBox().view(np.uint32))
        assert np.signbit(host.getBoundingBox()[0, 2]) == np.signbit(np.float32(first))


@pytest.mark.gpu
def test_the_library_takes_its_own_copy_at_set_time(trench_reference):
    D, gd, p, n, ld, rays = trench_reference["scene"]
    t = vr.TraceDisk(D)
    tp, tn = _tensors(p, n, ld)
    t.setGeometry(tp, tn, gd)
    tp.zero_()
    tn.zero_()
    _torch().cuda.synchronize()
    _configure(t, D, 0.1, PER, None, rays)
    t.apply()
    _assert_same(trench_reference["obs"], _observe(t))


@pytest.mark.gpu
def test_tensors_produced_on_a_side_stream_need_no_synchronize(trench_reference):
    """the rows are written by kernels queued on a non-default stream behind a few large matmuls; setGeometry, inside
    `with torch.cuda.stream(s)` and without any synchronize, must wait for them on the device"""
    torch = _torch()
    D, gd, p, n, ld, rays = trench_reference["scene"]
    hp, hn = torch.from_numpy(p).cuda(), torch.from_numpy(n).cuda()
    a = torch.randn(3072, 3072, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    t = vr.TraceDisk(D)
    with torch.cuda.stream(s):
        m = a
        for _ in range(4):
            m = (m @ a) * 1e-3
        keep = (m[0, 0] * 0.0).nan_to_num(0.0)  # (0, but only once the matmuls are through)
        tp, tn = hp + keep, hn + keep
        t.setGeometry(tp, tn, gd)
    _configure(t, D, 0.1, PER, None, rays)
    t.apply()
    _assert_same(trench_reference["obs"], _observe(t))
    s.synchronize()


@pytest.mark.gpu
def test_flux_tensor_is_ordered_on_the_consumers_stream(trench_reference):
    """getFluxTensor on a side stream, consumed there by a torch kernel without any synchronize: every element is the
    host vector's"""
    torch = _torch()
    D, gd, p, n, ld, rays = trench_reference["scene"]
    t = _device_run(D, gd, p, n, ld, 0.1, PER, None, rays)
    want = torch.from_numpy(t.getLocalData().getVectorData(0).copy())
    a = torch.randn(3072, 3072, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        m = a
        for _ in range(4):
            m = (m @ a) * 1e-3
        f = t.getFluxTensor()
        doubled = f * 2.0
    s.synchronize()
    assert f.device.type == "cuda" and f.dtype == torch.float32 and tuple(f.shape) == (p.shape[0],)
    assert torch.equal(f.cpu(), want)
    assert torch.equal(doubled.cpu(), want * 2.0)
    assert f.cpu().sum().item() == want.sum().item()


@pytest.mark.gpu
def test_flux_tensor_equals_the_host_chain():
    """raw / SOURCE / MAX x numNeighbors 0, 1, 2 x both labels of a two-label particle: element for element what
    getVectorData(i) -> normalizeFlux -> smoothFlux return on the same context"""
    torch = _torch()
    D, gd, p, n, ld, rays = _scene("trench3d")
    t = _device_run(D, gd, p, n, ld, 0.1, PER, None, rays, particle=vr.DiffuseCosineParticle(0.1, "flux", "cosine"))
    assert t.numData() == 2
    for idx in (0, 1):
        raw = t.getLocalData().getVectorData(idx)
        assert raw.any()
        for norm in (None, vr.NormalizationType.SOURCE, vr.NormalizationType.MAX):
            for k in (0, 1, 2):
                want = raw if norm is None else t.normalizeFlux(raw, norm)
                if k:
                    want = t.smoothFlux(want, k)
                got = t.getFluxTensor(idx, norm, k)
                assert got.device == torch.device("cuda", 0) and got.dtype == torch.float32 and tuple(got.shape) == (p.shape[0],)
                assert np.array_equal(got.cpu().numpy(), want), (idx, norm, k)


@pytest.mark.gpu
def test_flux_tensor_after_host_geometry_too(trench_reference):
    D, gd, p, n, ld, rays = trench_reference["scene"]
    t = _host_run(D, gd, p, n, ld, 0.1, PER, None, rays)
    got = t.getFluxTensor(0, vr.NormalizationType.SOURCE, 1).cpu().numpy()
    assert np.array_equal(got, t.smoothFlux(t.getFluxNormalized(vr.NormalizationType.SOURCE), 1))


@pytest.mark.gpu
def test_flux_tensor_refusals_leave_the_context_usable():
    torch = _torch()
    L = capi.load()
    D, gd, p, n, ld, rays = _scene("plane16")
    t = vr.TraceDisk(D)
    t.setGeometry(*_tensors(p, n, ld), gd)
    _configure(t, D, 0.5, PER, None, 10_000)
    with pytest.raises(vr.VrError, match="no result"):
        t.getFluxTensor()  # before apply
    t.apply()
    out = torch.empty(p.shape[0] + 1, dtype=torch.float32, device="cuda")
    ptr = C.c_void_p(out.data_ptr())
    assert L.vr_get_flux_device(t._h, 0, ptr, p.shape[0] + 1, capi.VR_NORM_NONE, 0, None) == capi.VR_E_INVALID  # wrong n
    assert b"size mismatch" in L.vr_last_error(t._h)
    with pytest.raises(vr.VrError, match="no such data label"):
        t.getFluxTensor(1)
    host = np.empty(p.shape[0], dtype=np.float32)
    assert L.vr_get_flux_device(t._h, 0, host.ctypes.data, p.shape[0], capi.VR_NORM_NONE, 0, None) == capi.VR_E_INVALID
    assert b"not device memory" in L.vr_last_error(t._h)
    assert np.array_equal(t.getFluxTensor().cpu().numpy(), t.getLocalData().getVectorData(0))


@pytest.mark.gpu
def test_switching_between_device_and_host_geometry_on_one_context():
    """device A (n1) -> device B (n2 != n1) -> host C -> device A again, one apply after each: every result is a fresh
    context's"""
    sticking, rays = 0.1, 50_000
    D, gdA, pA, nA, _, _ = _scene("trench3d")
    _, gdB, pB, nB, _, _ = _scene("ripple16")
    _, gdC, pC, nC, _, _ = _scene("sphere3d")
    assert len({pA.shape[0], pB.shape[0], pC.shape[0]}) == 3
    t = vr.TraceDisk(3)
    _configure(t, 3, sticking, PER, None, rays)
    for gd, p, n, on_device in ((gdA, pA, nA, True), (gdB, pB, nB, True), (gdC, pC, nC, False), (gdA, pA, nA, True)):
        if on_device:
            t.setGeometry(*_tensors(p, n, 3), gd)
        else:
            t.setGeometry(p, n, gd)
        t.setRunNumber(1)  # (every apply advances it: the fresh contexts trace run 1)
        t.apply()
        fresh = _host_run(3, gd, p, n, 3, sticking, PER, None, rays)
        a, b = _observe(fresh), _observe(t)
        a["info"].pop("bvhBuilds"), b["info"].pop("bvhBuilds")  # (the reused context has built more scenes)
        _assert_same(a, b)


@pytest.mark.gpu
def test_host_smoothing_after_a_device_set_reads_the_lazy_mirror(monkeypatch):
    D, gd, p, n, ld, rays = _scene("ripple16")
    host = _host_run(D, gd, p, n, ld, 0.1, PER, None, rays)
    dev = _device_run(D, gd, p, n, ld, 0.1, PER, None, rays)
    flux = host.getLocalData().getVectorData(0)
    on_device = host.smoothFlux(flux, 2)
    monkeypatch.setenv("VR_HOST_SMOOTH", "1")
    for k in (1, 2):
        assert np.array_equal(dev.smoothFlux(flux, k), host.smoothFlux(flux, k))
        assert np.array_equal(dev.getFluxTensor(0, None, k).cpu().numpy(), host.smoothFlux(flux, k))
    assert np.array_equal(dev.smoothFlux(flux, 2), on_device)


@pytest.mark.gpu
def test_host_build_after_a_device_set_reads_the_lazy_mirror(monkeypatch):
    D, gd, p, n, ld, rays = _scene("ripple16")
    monkeypatch.setenv("VR_HOST_BUILD", "1")
    a = _observe(_host_run(D, gd, p, n, ld, 0.1, PER, None, rays))
    b = _observe(_device_run(D, gd, p, n, ld, 0.1, PER, None, rays))
    _assert_same(a, b)


@pytest.mark.gpu
def test_refused_geometry_leaves_the_context_usable(trench_reference):
    torch = _torch()
    L = capi.load()
    D, gd, p, n, ld, rays = trench_reference["scene"]
    tp, tn = _tensors(p, n, 3)
    t = vr.TraceDisk(3)
    with pytest.raises(ValueError, match="dtype"):
        t.setGeometry(tp.double(), tn.double(), gd)
    wide_p, wide_n = torch.zeros(p.shape[0], 4, device="cuda"), torch.zeros(p.shape[0], 4, device="cuda")
    with pytest.raises(ValueError, match="contiguity"):
        t.setGeometry(wide_p[:, :3], wide_n[:, :3], gd)
    with pytest.raises(ValueError, match="device"):
        t.setGeometry(tp, tn.cpu(), gd)
    with pytest.raises(ValueError, match="device"):
        t.setGeometry(p, tn, gd)
    with pytest.raises(ValueError, match="shape"):
        t.setGeometry(tp, tn[:-1].contiguous(), gd)
    with pytest.raises(ValueError, match="shape"):
        t.setGeometry(tp[:, :2].contiguous(), tn[:, :2].contiguous(), gd)  # ld == 2 with D == 3
    # ... and the C entry point's own refusals
    ptr = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    assert L.vr_set_disks_device(t._h, ptr(tp), ptr(tn), p.shape[0], 2, gd, 0.0, 3, None) == capi.VR_E_INVALID
    assert b"D == 2" in L.vr_last_error(t._h)
    assert L.vr_set_disks_device(t._h, ptr(tp), ptr(tn), p.shape[0], 4, gd, 0.0, 3, None) == capi.VR_E_INVALID
    assert b"2 or 3" in L.vr_last_error(t._h)
    assert L.vr_set_disks_device(t._h, p.ctypes.data, n.ctypes.data, p.shape[0], 3, gd, 0.0, 3, None) == capi.VR_E_INVALID
    assert b"not device memory" in L.vr_last_error(t._h)
    # the context never saw a geometry: a valid call still works, and a refusal after it keeps it
    t.setGeometry(tp, tn, gd)
    assert L.vr_set_disks_device(t._h, p.ctypes.data, n.ctypes.data, p.shape[0], 3, gd, 0.0, 3, None) == capi.VR_E_INVALID
    _configure(t, D, 0.1, PER, None, rays)
    t.apply()
    _assert_same(trench_reference["obs"], _observe(t))


@pytest.mark.gpu
def test_cpp_facade_device_geometry(tmp_path):
    """tests/aux/facade_device_geometry.cpp: hipMalloc, fill, setGeometryDevice, apply, getFluxDevice — bit-equal to the
    host-geometry façade"""
    exe = tmp_path / "facade_device_geometry"
    lib = os.path.join(ROOT, "viennaray_amd")
    subprocess.check_call(["g++", "-O1"] + FACADE_FLAGS + [FACADE_SRC, "-o", str(exe), "-L", lib, "-lviennaray_amd",
                                                          "-L", "/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib,
                                                          "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "facade device geometry ok" in out.stdout, out.stdout + out.stderr
