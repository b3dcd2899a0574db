"""Host-side mirror of the reference front-end for the accelerated path.

Same names, argument meaning and error behaviour as `viennaray::Trace<T,D>`,
`TraceDisk`, `TraceTriangle`, `DiffuseParticle`, `SpecularParticle`,
`TracingData` (reference: include/viennaray/rayTrace.hpp:15-180,
rayTraceDisk.hpp:13-224, rayTraceTriangle.hpp:13-154, rayParticle.hpp:126-204,
rayTracingData.hpp:16-219), driving the C ABI in include/viennaray_amd.h.
The C++ façade with the reference's exact spelling lives in
include/viennaray_amd/*.hpp; this module exists so the parity tests read like
the reference's tests.
"""
import ctypes as C
import enum
import math

import numpy as np

from . import capi
from .capi import VrError, TraceInfoPOD, ParticlePOD, GatherSpecPOD, GatherAdaptiveInfoPOD, GatherLawsPOD, GatherEnergyPOD


class BoundaryCondition(enum.IntEnum):  # rayBoundary.hpp:10-14
    REFLECTIVE_BOUNDARY = 0
    PERIODIC_BOUNDARY = 1
    IGNORE_BOUNDARY = 2


class TraceDirection(enum.IntEnum):  # rayUtil.hpp:40-47
    POS_X = 0
    NEG_X = 1
    POS_Y = 2
    NEG_Y = 3
    POS_Z = 4
    NEG_Z = 5


class NormalizationType(enum.IntEnum):  # rayUtil.hpp:38
    SOURCE = 0
    MAX = 1


class GatherMode(enum.IntEnum):  # Trace.gatherFlux (VR_GATHER_*, include/viennaray_amd.h)
    NORMAL = 0  # samples follow the cosine law about the primitive's normal
    SOURCE = 1  # samples follow the source's power-cosine law about the direction to the source plane


class GatherReflection(enum.IntEnum):  # Trace.gatherPaths (VR_GATHER_REFLECT_*, include/viennaray_amd.h)
    SPECULAR = 0  # a vertex reflects the path into the mirror direction
    DIFFUSE = 1   # a vertex re-emits it by the cosine law about the normal hit


class GatherEnd(enum.IntEnum):  # how a gathered path ended (VR_GATHER_END_*, include/viennaray_amd.h): debugGather*Path's "end"
    MISS = 0      # reached the source plane
    IGNORED = 1   # left through an IGNORE wall
    WALL = 2      # stopped on a wall: the boundary-hit budget is spent
    BACK = 4      # hit a primitive on its back side
    BOUNCES = 5   # a front-side hit with maxBounces bounces made
    ABSORBED = 6  # a front-side hit that took the throughput to 0
    ENERGY = 7    # gatherEnergy's cut: the arrival energy entered the zero region of energyYield


class TracingDataMergeEnum(enum.IntEnum):  # rayTracingData.hpp:10-14
    SUM = 0
    APPEND = 1
    AVERAGE = 2


class DiffuseParticle:
    """rayParticle.hpp:126-163"""
    kind = 0

    def __init__(self, stickingProbability, dataLabel, materialSticking=None):
        self.stickingProbability = float(stickingProbability)
        self.dataLabel = dataLabel
        self.materialSticking = dict(materialSticking or {})

    def getSourceDistributionPower(self):
        return 1.0

    def getLocalDataLabels(self):
        return [self.dataLabel]


class SpecularParticle:
    """rayParticle.hpp:165-204"""
    kind = 1

    def __init__(self, stickingProbability, sourcePower, dataLabel, materialSticking=None):
        self.stickingProbability = float(stickingProbability)
        self.sourcePower = float(sourcePower)
        self.dataLabel = dataLabel
        self.materialSticking = dict(materialSticking or {})

    def getSourceDistributionPower(self):
        return self.sourcePower

    def getLocalDataLabels(self):
        return [self.dataLabel]


class ConedCosineParticle:
    """Plug-in particle of the device registry (vr_particles.hpp): collects like SpecularParticle,
    reflects with ReflectionConedCosine(maxConeAngle) (rayReflection.hpp:52-120)."""
    kind = 2

    def __init__(self, stickingProbability, sourcePower, coneAngle, dataLabel, materialSticking=None,
                 meanFreePath=-1.0):
        self.stickingProbability = float(stickingProbability)
        self.sourcePower = float(sourcePower)
        self.coneAngle = float(coneAngle)
        self.dataLabel = dataLabel
        self.materialSticking = dict(materialSticking or {})
        self.meanFreePath = float(meanFreePath)

    def getSourceDistributionPower(self):
        return self.sourcePower

    def getMeanFreePath(self):
        return self.meanFreePath

    def getLocalDataLabels(self):
        return [self.dataLabel]


class DiffuseCosineParticle:
    """Plug-in particle with TWO data labels: label 0 += w (like DiffuseParticle), label 1 += w * max(0, -d.n)."""
    kind = 3

    def __init__(self, stickingProbability, dataLabel, cosineLabel, materialSticking=None, meanFreePath=-1.0):
        self.stickingProbability = float(stickingProbability)
        self.dataLabels = [dataLabel, cosineLabel]
        self.materialSticking = dict(materialSticking or {})
        self.meanFreePath = float(meanFreePath)

    def getSourceDistributionPower(self):
        return 1.0

    def getMeanFreePath(self):
        return self.meanFreePath

    def getLocalDataLabels(self):
        return list(self.dataLabels)


class CoverageStickingParticle:
    """Plug-in particle reading Trace.setGlobalData: a DiffuseParticle whose sticking falls with the coverage of the
    primitive it meets, sticking * (1 - globalData.getVectorData(coverageVector)[primID]) — the host form returns
    that as the first member of surfaceReflection (rayParticle.hpp:44-50)."""
    kind = 4

    def __init__(self, stickingProbability, dataLabel, coverageVector=0, materialSticking=None):
        self.stickingProbability = float(stickingProbability)
        self.dataLabel = dataLabel
        self.coverageVector = int(coverageVector)
        self.materialSticking = dict(materialSticking or {})
        self.params = [float(self.coverageVector)]

    def getSourceDistributionPower(self):
        return 1.0

    def getLocalDataLabels(self):
        return [self.dataLabel]


class UserModelParticle:
    """A particle whose device model was registered at run time (Trace.registerParticleModel): `kind` is what the
    registration returned, `dataLabels` one label per data label of the model, `params` the model's parameters."""

    def __init__(self, kind, stickingProbability, dataLabels, sourcePower=1.0, params=(), materialSticking=None,
                 meanFreePath=-1.0):
        self.kind = int(kind)
        self.stickingProbability = float(stickingProbability)
        self.dataLabels = list(dataLabels)
        self.sourcePower = float(sourcePower)
        self.params = [float(v) for v in params]
        self.materialSticking = dict(materialSticking or {})
        self.meanFreePath = float(meanFreePath)

    def getSourceDistributionPower(self):
        return self.sourcePower

    def getLocalDataLabels(self):
        return list(self.dataLabels)


class SourceGrid:
    """raySourceGrid.hpp: explicit ray origins (createSourceGrid, rayUtil.hpp:564-611); the direction
    comes from the particle's cosine power."""

    def __init__(self, points):
        self.points = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)

    def getNumPoints(self):
        return self.points.shape[0]


class SourceModel:
    """A user Source (raySource.hpp:10-19) as device code: `source` is HIP text defining `struct VrUserSource` (kHasWeight,
    sample<D>(ctx, idx, draw, org, dir, weight); include/viennaray_amd.h: vr_register_source_model), compiled into the ray
    generator when a tracer's setSource(model) first sees the text (the tracer keeps the registration: one model object
    may serve any number of tracers, one after the other or side by side).  params: up to 16 floats the model reads as ctx.params; table:
    one float32 table it reads as ctx.table[0 .. ctx.tableCount) — a host array, or a 1-D contiguous float32 torch tensor
    on the tracer's device, which stays there; numRays: 0 keeps numRaysPerPoint / numRaysFixed over the primitives, > 0
    is the source's own ray count; hasWeight: the text's kHasWeight."""

    def __init__(self, name, source, params=(), table=None, numRays=0, hasWeight=False):
        if not isinstance(source, str) or not source.strip():
            raise ValueError("SourceModel: source must be the HIP text of struct VrUserSource")
        self.name = str(name)
        self.source = source
        self.hasWeight = bool(hasWeight)
        self.params = self._checked_params(params)
        self.table = self._checked_table(table)
        self.numRays = int(numRays)
        if not 0 <= self.numRays <= 0xFFFFFFFF:
            raise ValueError("SourceModel: numRays must be 0 .. 2^32 - 1")

    @staticmethod
    def _checked_params(params):
        a = np.ascontiguousarray(params, dtype=np.float32)
        if a.ndim != 1 or a.size > capi.VR_SOURCE_PARAMS:
            raise ValueError(f"SourceModel: params: at most {capi.VR_SOURCE_PARAMS} floats in one dimension, got shape {a.shape}")
        return a

    @staticmethod
    def _checked_table(table):
        """None, a device tensor (checked against the tracer's device when it is set) or a host float32 vector"""
        if table is None:
            return None
        if hasattr(table, "data_ptr"):  # a torch tensor: handed over where it is, or refused
            if not _on_any_device(table):
                raise ValueError("SourceModel: table: device: a torch tensor must be on the tracer's device "
                                 "(pass a host table as a numpy array)")
            return table
        a = np.asarray(table)
        if a.dtype != np.float32 and not isinstance(table, (list, tuple)):
            raise ValueError(f"SourceModel: table: dtype: {a.dtype}, a table is float32")
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.ndim != 1:
            raise ValueError(f"SourceModel: table: shape: {a.shape}, a table has one dimension")
        return a


class TracingData:
    """rayTracingData.hpp:16-219: labelled vectors and scalars with a merge type each.  The
    device path fills vector 0 of Trace.getLocalData() (merge type SUM)."""

    def __init__(self):
        self._vectors, self._vlabels, self._vmerge = [], [], []
        self._scalars, self._slabels, self._smerge = [], [], []

    def setNumberOfVectorData(self, n):
        self._vectors = [np.zeros(0, dtype=np.float32) for _ in range(n)]
        self._vlabels = ["vectorData"] * n
        self._vmerge = [TracingDataMergeEnum.SUM] * n

    def setNumberOfScalarData(self, n):
        self._scalars = [0.0] * n
        self._slabels = ["scalarData"] * n
        self._smerge = [TracingDataMergeEnum.SUM] * n

    def setScalarData(self, num, value, label="scalarData"):
        self._scalars[num] = float(value)
        self._slabels[num] = label

    def setVectorData(self, num, data, label="vectorData", value=None):
        """setVectorData(num, array, label) or setVectorData(num, size, label, value=v)"""
        if value is not None:
            data = np.full(int(data), value, dtype=np.float32)
        self._vectors[num] = np.asarray(data, dtype=np.float32)
        self._vlabels[num] = label

    def appendVectorData(self, num, data):
        self._vectors[num] = np.concatenate([self._vectors[num], np.asarray(data, dtype=np.float32)])

    def resizeAllVectorData(self, size, val=0.0):
        self._vectors = [np.full(int(size), val, dtype=np.float32) for _ in self._vectors]

    def setVectorMergeType(self, num, m):
        self._vmerge[num] = TracingDataMergeEnum(m)

    def setScalarMergeType(self, num, m):
        self._smerge[num] = TracingDataMergeEnum(m)

    def getVectorData(self, key=0):
        if isinstance(key, str):
            i = self.getVectorDataIndex(key)
            if i < 0:
                raise KeyError("Can not find vector data label in TracingData.")
            key = i
        return self._vectors[key]

    def getScalarData(self, key=0):
        if isinstance(key, str):
            i = self.getScalarDataIndex(key)
            if i < 0:
                raise KeyError("Can not find scalar data label in TracingData.")
            key = i
        return self._scalars[key]

    def getVectorDataLabel(self, i):
        return self._vlabels[i] if i < len(self._vlabels) else ""

    def getScalarDataLabel(self, i):
        return self._slabels[i] if i < len(self._slabels) else ""

    def getVectorDataIndex(self, label):
        return self._vlabels.index(label) if label in self._vlabels else -1

    def getScalarDataIndex(self, label):
        return self._slabels.index(label) if label in self._slabels else -1

    def getVectorMergeType(self, num):
        return self._vmerge[num]

    def getScalarMergeType(self, num):
        return self._smerge[num]


def _fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _on_any_device(x):
    """a tensor that is not host memory, whatever device it lives on, by duck typing (this module does not import torch):
    what sends a setter down its device path"""
    return hasattr(x, "data_ptr") and getattr(getattr(x, "device", None), "type", "cpu") != "cpu"


def _check_device_tensor(what, name, x, device, dtype, shapes):
    """a tensor handed over where it is must be on the tracer's device, of the one dtype, contiguous and of one of the
    shapes (None: any size): anything else raises ValueError — nothing is copied through the host behind the caller's
    back"""
    if not (hasattr(x, "data_ptr") and bool(getattr(x, "is_cuda", False))):
        raise ValueError(f"{what}: device: {name} is not a device tensor while another argument is "
                         "(all on the device, or all on the host)")
    if x.device.index != device:
        raise ValueError(f"{what}: device: {name} is on {x.device}, the tracer on device {device}")
    if str(x.dtype) != dtype:
        raise ValueError(f"{what}: dtype: {name} is {x.dtype}, device tensors must be {dtype}")
    shape = tuple(x.shape)
    if not any(len(shape) == len(w) and all(b is None or a == b for a, b in zip(shape, w)) for w in shapes):
        raise ValueError(f"{what}: shape: {name} is {shape}")
    if not x.is_contiguous():
        raise ValueError(f"{what}: contiguity: {name} is not contiguous (strides {tuple(x.stride())})")


class Trace:
    """rayTrace.hpp:15-180 (NumericType = float)."""

    def __init__(self, D=3, device=0):
        self.D = D
        self._L = capi.load()
        h = C.c_void_p()
        rc = self._L.vr_create(C.byref(h), device)
        if rc != capi.VR_OK:
            raise VrError("vr_create failed: no usable HIP device (the accelerated path has no CPU fallback)")
        self._h = h
        self._device = int(device)
        self._particle = None
        self._sourceIds = {}  # (text, hasWeight) of a SourceModel -> its id on this context
        self._localData = TracingData()
        self._n = 0

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._L.vr_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def _check(self, rc):
        if rc != capi.VR_OK:
            raise VrError(self._L.vr_last_error(self._h).decode())

    # --- setters (rayTrace.hpp:41-121) --------------------------------------
    def _pod(self, particle, keep):
        pod = ParticlePOD()
        pod.kind = particle.kind
        pod.sticking = particle.stickingProbability
        pod.sourcePower = particle.getSourceDistributionPower()
        pod.coneAngle = getattr(particle, "coneAngle", 0.0)
        pod.meanFreePath = getattr(particle, "meanFreePath", -1.0)
        for k, v in enumerate(getattr(particle, "params", [])[:8]):
            pod.params[k] = v
        ms = particle.materialSticking
        if ms:
            ids = (C.c_int32 * len(ms))(*ms.keys())
            vals = (C.c_float * len(ms))(*ms.values())
            pod.numMaterialSticking = len(ms)
            pod.materialIds = ids
            pod.materialSticking = vals
            keep.append((ids, vals))
        return pod

    def setParticleType(self, particle):
        self._particle = particle
        self._particles = [particle]
        keep = []
        pod = self._pod(particle, keep)
        self._check(self._L.vr_set_particle(self._h, C.byref(pod)))
        del keep

    def setParticleTypes(self, particles):
        """Several particles traced in ONE apply() (the reference's gpu::Trace keeps a particle list,
        gpu/raygTrace.hpp:163-248): every particle sees the same seed, particles with the same source
        distribution share one generator pass; getLocalData() holds particle 0's labels, then particle 1's, ..."""
        particles = list(particles)
        keep = []
        arr = (ParticlePOD * len(particles))(*[self._pod(q, keep) for q in particles])
        self._check(self._L.vr_set_particles(self._h, arr, len(particles)))
        self._particle = particles[0]
        self._particles = particles
        del keep

    def registerParticleModel(self, source, numData=1, needsFull=False, name="user", numState=0):
        """vr_register_particle_model: HIP source of `struct VrUserModel` -> the kind id of a UserModelParticle.
        numState = the model's kStateWords (1 .. 4: a stateful model with init / surface_reflection / collide hooks,
        vr_register_particle_model_ex; it implies needsFull)"""
        k = C.c_int32(0)
        if numState:
            self._check(self._L.vr_register_particle_model_ex(self._h, name.encode(), source.encode(), int(numData),
                                                              int(numState), 1 if needsFull else 0, C.byref(k)))
        else:
            self._check(self._L.vr_register_particle_model(self._h, name.encode(), source.encode(), int(numData),
                                                           1 if needsFull else 0, C.byref(k)))
        return int(k.value)

    def setGlobalData(self, data):
        """rayTrace.hpp:141: a TracingData (or a list of per-primitive arrays) the device particle models may read"""
        vecs = data._vectors if isinstance(data, TracingData) else list(data)
        for k, v in enumerate(vecs):  # (before anything is dropped: a refusal leaves the previous data in force)
            if _on_any_device(v):
                _check_device_tensor("setGlobalData", f"vector {k}", v, self._device, "torch.float32", [(None,)])
        self._check(self._L.vr_set_global_data(self._h, 0, None, 0))
        for k, v in enumerate(vecs):
            if _on_any_device(v):
                # a float32 tensor on the tracer's device stays there (vr_set_global_data_device): copied into place
                # by a kernel ordered behind the current torch stream, which may overwrite the tensor afterwards
                self._check(self._L.vr_set_global_data_device(self._h, k, C.c_void_p(v.data_ptr()), int(v.numel()),
                                                              C.c_void_p(self._torch_stream())))
                continue
            a = np.ascontiguousarray(v, dtype=np.float32)
            self._check(self._L.vr_set_global_data(self._h, k, _fptr(a), a.size))
        if isinstance(data, TracingData) and data._scalars:
            sc = np.ascontiguousarray(data._scalars, dtype=np.float32)
            self._check(self._L.vr_set_global_scalars(self._h, _fptr(sc), sc.size))
        else:  # (no scalars in the new data: the previous ones must not linger on the device)
            self._check(self._L.vr_set_global_scalars(self._h, None, 0))
        self._globalData = data

    def setGlobalVector(self, k, v):
        """One vector of the global data, the others untouched: a float32 tensor on the tracer's device (set on the
        device, as in setGlobalData) or a host array; None drops vector k and those behind it."""
        if v is None:
            self._check(self._L.vr_set_global_data(self._h, int(k), None, 0))
        elif _on_any_device(v):
            _check_device_tensor("setGlobalVector", f"vector {k}", v, self._device, "torch.float32", [(None,)])
            self._check(self._L.vr_set_global_data_device(self._h, int(k), C.c_void_p(v.data_ptr()), int(v.numel()),
                                                          C.c_void_p(self._torch_stream())))
        else:
            a = np.ascontiguousarray(v, dtype=np.float32)
            self._check(self._L.vr_set_global_data(self._h, int(k), _fptr(a), a.size))

    def _torch_stream(self):
        import torch
        return torch.cuda.current_stream(torch.device("cuda", self._device)).cuda_stream

    def getGlobalData(self):
        return getattr(self, "_globalData", None)

    def getParticleTraceInfo(self, q):
        pod = TraceInfoPOD()
        self._check(self._L.vr_get_particle_trace_info(self._h, int(q), C.byref(pod)))
        return pod

    def setUseWdist(self, on=True):
        """VIENNARAY_USE_WDIST as a run-time switch (rayTraceKernel.hpp:258-296)"""
        self._check(self._L.vr_set_use_wdist(self._h, int(bool(on))))

    def setSource(self, source):
        """rayTrace.hpp:53-56.  SourceGrid runs natively in the generator kernel; a SourceModel is compiled into the
        generator and sampled on the device (None: back to SourceRandom); the rays of a host-callback source
        (getOriginAndDirection(idx, rng) evaluated by the caller) go through setHostRays."""
        if isinstance(source, SourceGrid):
            self._check(self._L.vr_set_source_grid(self._h, _fptr(source.points), source.points.shape[0]))
            return
        if source is None or isinstance(source, SourceModel):
            return self._setSourceModel(source)
        raise VrError("setSource: host-callback sources go through setHostRays(origins, directions, draws)")

    def registerSourceModel(self, name, source, hasWeight=False):
        """vr_register_source_model: HIP text of `struct VrUserSource` -> the id vr_set_source_model takes"""
        k = C.c_int32(-1)
        self._check(self._L.vr_register_source_model(self._h, str(name).encode(), source.encode(),
                                                     capi.VR_SOURCE_HAS_WEIGHT if hasWeight else 0, C.byref(k)))
        return int(k.value)

    def _setSourceModel(self, model):
        """A SourceModel becomes the source (None: back to SourceRandom).  Everything is checked before anything is set:
        a refusal leaves the previous source, and its table, in force."""
        if model is None:
            self._check(self._L.vr_set_source_model(self._h, -1, None, 0, None, 0, 0))
            return
        params = SourceModel._checked_params(model.params)
        table = SourceModel._checked_table(model.table)
        onDevice = table is not None and hasattr(table, "data_ptr")
        if onDevice:
            _check_device_tensor("setSource", "table", table, self._device, "torch.float32", [(None,)])
        # the registration belongs to THIS tracer's context and to the text: kept here, by content, so that a model object
        # may outlive a tracer or serve several, and a model object rebuilt for new parameters registers nothing again
        key = (model.source, model.hasWeight)
        if key not in self._sourceIds:
            self._sourceIds[key] = self.registerSourceModel(model.name, model.source, model.hasWeight)
        host = None if (onDevice or table is None) else table
        self._check(self._L.vr_set_source_model(self._h, self._sourceIds[key], _fptr(params) if params.size else None, params.size,
                                                _fptr(host) if host is not None and host.size else None,
                                                host.size if host is not None else 0, int(model.numRays)))
        if onDevice:
            # a float32 tensor on the tracer's device stays there (vr_set_source_model_table_device): copied by the
            # library behind the current torch stream, which may overwrite the tensor afterwards
            self._check(self._L.vr_set_source_model_table_device(self._h, C.c_void_p(table.data_ptr()), int(table.numel()),
                                                                 C.c_void_p(self._torch_stream())))

    def setSourceModelTable(self, table):
        """The table of the source model in force alone: a host float32 vector is not taken here (set the model again);
        a float32 1-D contiguous tensor on the tracer's device is copied on the device.  Anything else raises
        ValueError and the previous table stays."""
        if not hasattr(table, "data_ptr") or not _on_any_device(table):
            raise ValueError("setSourceModelTable: device: the table must be a torch tensor on the tracer's device")
        _check_device_tensor("setSourceModelTable", "table", table, self._device, "torch.float32", [(None,)])
        self._check(self._L.vr_set_source_model_table_device(self._h, C.c_void_p(table.data_ptr()), int(table.numel()),
                                                             C.c_void_p(self._torch_stream())))

    def setHostRays(self, origins, directions, draws=None, weights=None, sourceArea=None):
        """Rays of a host-callback Source (raySource.hpp:10-19): origin, direction, engine outputs consumed and —
        if the source overrides them — getInitialRayWeight(idx) per ray and getSourceArea()."""
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3)
        assert o.shape == d.shape
        k = None
        if draws is not None:
            k = np.ascontiguousarray(draws, dtype=np.uint32)
            assert k.size == o.shape[0]
        self._check(self._L.vr_set_host_rays(self._h, _fptr(o), _fptr(d),
                                             k.ctypes.data_as(C.POINTER(C.c_uint32)) if k is not None else None,
                                             o.shape[0]))
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float32)
            assert w.size == o.shape[0]
            self._check(self._L.vr_set_host_ray_weights(self._h, _fptr(w), w.size))
        if sourceArea is not None or hasattr(self._L, "vr_set_source_area"):
            self._check(self._L.vr_set_source_area(self._h, float(sourceArea) if sourceArea is not None else 0.0))

    def setSurfaceSource(self, positions, normals, weights, sourceArea, sourceOffset):
        """gpu/raygTrace.hpp:267-286: the rays start on the given points (numRaysFixed if set, else numRaysPerPoint,
        rays per point), leave along a cosine distribution about each point's normal from position + unit normal *
        sourceOffset and carry the point's weight; sampled on the device.  normalizeFlux(SOURCE) uses sourceArea.
        Three torch tensors on the tracer's device (positions and normals [n, 2] or [n, 3] float32, weights [n] float32,
        contiguous) are handed over where they are (vr_set_surface_source_device): packed and validated by one kernel
        behind the current torch stream.  Tensors on a device that cannot go that way raise ValueError."""
        if _on_any_device(positions) or _on_any_device(normals) or _on_any_device(weights):
            return self._setSurfaceSourceDevice(positions, normals, weights, sourceArea, sourceOffset)
        q = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        m = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
        if m.shape != q.shape or w.size != q.shape[0]:
            raise VrError("setSurfaceSource: one normal and one weight per position")
        self._check(self._L.vr_set_surface_source(self._h, _fptr(q), _fptr(m), _fptr(w), q.shape[0],
                                                  float(sourceArea), float(sourceOffset)))

    def _setSurfaceSourceDevice(self, positions, normals, weights, sourceArea, sourceOffset):
        cols = [(None, 2), (None, 3)] if self.D == 2 else [(None, 3)]
        _check_device_tensor("setSurfaceSource", "positions", positions, self._device, "torch.float32", cols)
        n, ld = int(positions.shape[0]), int(positions.shape[1])
        _check_device_tensor("setSurfaceSource", "normals", normals, self._device, "torch.float32", [(n, ld)])
        _check_device_tensor("setSurfaceSource", "weights", weights, self._device, "torch.float32", [(n,)])
        self._check(self._L.vr_set_surface_source_device(
            self._h, C.c_void_p(positions.data_ptr()), C.c_void_p(normals.data_ptr()), C.c_void_p(weights.data_ptr()),
            n, ld, float(sourceArea), float(sourceOffset), C.c_void_p(self._torch_stream())))

    def clearSurfaceSource(self):
        """gpu/raygTrace.hpp:288-297"""
        self._check(self._L.vr_set_surface_source(self._h, None, None, None, 0, 0.0, 0.0))

    def reserveRays(self, n):
        """Size the HBM ray stream for applies of up to n rays (apply() per time step with a growing count)."""
        self._check(self._L.vr_reserve_rays(self._h, int(n)))

    def resetSource(self):
        """rayTrace.hpp:58-61 (also drops a surface source)"""
        self._check(self._L.vr_set_source_grid(self._h, None, 0))
        self._check(self._L.vr_set_source_area(self._h, 0.0))

    def setBoundaryConditions(self, bcs):
        a = (C.c_int32 * len(bcs))(*[int(b) for b in bcs])
        self._check(self._L.vr_set_boundary_conditions(self._h, a, len(bcs)))

    def setNumberOfRaysPerPoint(self, n):
        self._check(self._L.vr_set_number_of_rays_per_point(self._h, int(n)))

    def setNumberOfRaysFixed(self, n):
        self._check(self._L.vr_set_number_of_rays_fixed(self._h, int(n)))

    def setMaxReflections(self, n):
        self._check(self._L.vr_set_max_reflections(self._h, int(n)))

    def setMaxBoundaryHits(self, n):
        self._check(self._L.vr_set_max_boundary_hits(self._h, int(n)))

    def setSourceDirection(self, d):
        self._check(self._L.vr_set_source_direction(self._h, int(d)))

    def setPrimaryDirection(self, d):
        a = np.ascontiguousarray(d, dtype=np.float32)
        self._check(self._L.vr_set_primary_direction(self._h, _fptr(a)))

    def setUseRandomSeeds(self, b):
        self._check(self._L.vr_set_use_random_seeds(self._h, int(bool(b))))

    def setRngSeed(self, s):
        self._check(self._L.vr_set_rng_seed(self._h, int(s)))

    def setMaterialIds(self, ids):
        """rayGeometry.hpp:17-24.  An int32 tensor on the tracer's device (1-D, contiguous) stays there
        (vr_set_material_ids_device); any other device tensor raises ValueError."""
        if _on_any_device(ids):
            _check_device_tensor("setMaterialIds", "ids", ids, self._device, "torch.int32", [(None,)])
            self._check(self._L.vr_set_material_ids_device(self._h, C.c_void_p(ids.data_ptr()), int(ids.numel()),
                                                           C.c_void_p(self._torch_stream())))
            return
        a = np.ascontiguousarray(ids, dtype=np.int32)
        self._check(self._L.vr_set_material_ids(self._h, a.ctypes.data_as(C.POINTER(C.c_int32)), a.size))

    # --- extensions used by the multi-GPU driver and the tests ---------------
    def setRunNumber(self, r):
        self._check(self._L.vr_set_run_number(self._h, int(r)))

    def getRunNumber(self):
        v = C.c_uint32(0)
        self._check(self._L.vr_get_run_number(self._h, C.byref(v)))
        return int(v.value)

    def skipApply(self):
        """What an apply() does to the run number (rayTraceDisk.hpp:54) without tracing: a rank
        whose ray shard is empty stays in step with the others' seeds."""
        self.setRunNumber(self.getRunNumber() + 1)

    def setRayRange(self, first, count):
        self._check(self._L.vr_set_ray_range(self._h, int(first), int(count)))

    def setWorldSize(self, world):
        """Ranks whose accumulators will be summed: head-room of the accumulator-overflow check (vr_set_world_size)."""
        self._check(self._L.vr_set_world_size(self._h, int(world)))

    # --- run ---------------------------------------------------------------
    def apply(self, collect=True):
        """collect=False leaves the flux on the device (getFluxTensor / getFluxNormalized fetch it): getLocalData() is
        not filled"""
        if self._particle is None:
            # checkSettings (rayTraceDisk.hpp:197-200)
            raise VrError("No particle was specified in rayTrace. Aborting.")
        self._check(self._L.vr_apply(self._h))
        if collect:
            self._collect()

    def applySharded(self, rank, world, reduce_fn=None, user=None):
        """vr_apply_sharded: this rank's share of the rays, then `reduce_fn(user, devPtr, count, stream)` (a
        ctypes function pointer, e.g. vr_rccl_allreduce) sums accumulators and counters over the ranks."""
        if self._particle is None:
            raise VrError("No particle was specified in rayTrace. Aborting.")
        fn = C.cast(reduce_fn, C.c_void_p) if reduce_fn is not None else None
        self._check(self._L.vr_apply_sharded(self._h, int(rank), int(world), fn, user))
        self._collect()

    def applyPrepare(self):
        self._check(self._L.vr_apply_prepare(self._h))

    def applyLaunch(self):
        self._check(self._L.vr_apply_launch(self._h))

    def applyFinish(self, collect=True):
        self._check(self._L.vr_apply_finish(self._h))
        if collect:
            self._collect()

    def _collect(self):
        labels = [l for q in getattr(self, "_particles", [self._particle]) for l in q.getLocalDataLabels()]
        self._localData.setNumberOfVectorData(len(labels))
        for l, label in enumerate(labels):
            out = np.empty(self._n, dtype=np.float32)
            self._check(self._L.vr_get_flux_data(self._h, l, _fptr(out), self._n))
            self._localData.setVectorData(l, out, label)

    def numData(self):
        return int(self._L.vr_num_data(self._h))

    def getLocalData(self):
        return self._localData

    def getFluxF64(self):
        out = np.empty(self._n, dtype=np.float64)
        self._check(self._L.vr_get_flux_f64(self._h, out.ctypes.data_as(C.POINTER(C.c_double)), self._n))
        return out

    def getRayTraceInfo(self):
        pod = TraceInfoPOD()
        self._check(self._L.vr_get_trace_info(self._h, C.byref(pod)))
        return pod

    def traceMode(self):
        """trace_kernel variant of the last prepare: 0 general, 1 absorbing/flat, 2 absorbing/structured"""
        v = C.c_int32(0)
        self._check(self._L.vr_get_trace_mode(self._h, C.byref(v)))
        return int(v.value)

    def normalizeFlux(self, flux, norm=NormalizationType.SOURCE):
        f = np.ascontiguousarray(flux, dtype=np.float32).copy()
        self._check(self._L.vr_normalize_flux(self._h, _fptr(f), f.size, int(norm)))
        return f

    def getFluxNormalized(self, norm=NormalizationType.SOURCE):
        """raw flux -> normalizeFlux fused on the device (one download)"""
        out = np.empty(self._n, dtype=np.float32)
        self._check(self._L.vr_get_flux_normalized(self._h, _fptr(out), self._n, int(norm)))
        return out

    def getFluxTensor(self, dataIdx=0, norm=None, numNeighbors=0):
        """The flux of data label `dataIdx` as a new torch.float32 tensor on the context's device, in the caller's
        primitive order: raw (norm=None) or normalizeFlux(norm), then smoothFlux(numNeighbors) if numNeighbors > 0 —
        computed and left on the device (vr_get_flux_device), ordered on the current torch stream: no host copy, and
        without smoothing no synchronisation."""
        import torch
        dev = torch.device("cuda", self._device)
        out = torch.empty(self._n, dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        self._check(self._L.vr_get_flux_device(self._h, int(dataIdx), C.c_void_p(out.data_ptr()), self._n,
                                               capi.VR_NORM_NONE if norm is None else int(norm), int(numNeighbors),
                                               C.c_void_p(stream)))
        return out

    # --- per-primitive values at the caller's points (vr_map_to_points*, include/viennaray_amd.h has the definition) ----
    def _mapArgs(self, what, points, normals, radius):
        """(device?, points, normals, m, ld, radius): float32 torch tensors on the tracer's device go as they are
        (anything else about a tensor raises ValueError), host arrays as contiguous [m, 3] float32"""
        radius = 2.0 * getattr(self, "_gridDelta", 0.0) if radius is None else float(radius)
        if _on_any_device(points) or (normals is not None and _on_any_device(normals)) or hasattr(points, "data_ptr"):
            cols = [(None, 2), (None, 3)] if self.D == 2 else [(None, 3)]
            _check_device_tensor(what, "points", points, self._device, "torch.float32", cols)
            if normals is not None:
                _check_device_tensor(what, "normals", normals, self._device, "torch.float32", [tuple(points.shape)])
            return True, points, normals, int(points.shape[0]), int(points.shape[1]), radius
        p = np.asarray(points, dtype=np.float32)
        p = p.reshape(-1, p.shape[-1]) if p.ndim == 2 else p.reshape(-1, 3)
        q = None if normals is None else np.asarray(normals, dtype=np.float32).reshape(p.shape)
        if p.shape[1] == 2:  # 2-D rows: z := 0, as setGeometry does
            p = np.concatenate([p, np.zeros((p.shape[0], 1), np.float32)], axis=1)
            q = None if q is None else np.concatenate([q, np.zeros((q.shape[0], 1), np.float32)], axis=1)
        p = np.ascontiguousarray(p)
        q = None if q is None else np.ascontiguousarray(q)
        return False, p, q, int(p.shape[0]), 3, radius

    def mapToPoints(self, values, points, normals=None, radius=None):
        """One float per primitive (caller's order) mapped to the m query points: the mean of `values` over the primitive
        centres within `radius` (None: 2 * gridDelta) weighted by (1 - d / radius) * max(0, n_j . normal_i) — no gate
        without normals — or the value of the nearest centre where that sum of weights is not positive (radius 0,
        nothing in range, every normal facing away).  Plain Euclidean distances, no periodic wrap; 2-D scenes ignore z.
        float32 torch tensors on the tracer's device in give a tensor out, computed on the device and ordered on the
        current torch stream (vr_map_to_points_device; a tensor of another dtype or device, or a non-contiguous one,
        raises ValueError); host arrays in give a numpy array out (vr_map_to_points).  Needs the scene build of the
        geometry in force: call apply() (or applyPrepare()) first."""
        dev, p, q, m, ld, radius = self._mapArgs("mapToPoints", points, normals, radius)
        if dev:
            import torch
            _check_device_tensor("mapToPoints", "values", values, self._device, "torch.float32", [(None,)])
            out = torch.empty(m, dtype=torch.float32, device=p.device)
            self._check(self._L.vr_map_to_points_device(
                self._h, C.c_void_p(values.data_ptr()), int(values.shape[0]), C.c_void_p(p.data_ptr()),
                C.c_void_p(q.data_ptr()) if q is not None else None, m, ld, radius, C.c_void_p(out.data_ptr()),
                C.c_void_p(self._torch_stream())))
            return out
        if hasattr(values, "data_ptr"):
            raise ValueError("mapToPoints: device: values is a tensor while points is a host array "
                             "(all on the device, or all on the host)")
        v = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
        out = np.empty(m, dtype=np.float32)
        self._check(self._L.vr_map_to_points(self._h, _fptr(v), v.size, _fptr(p), _fptr(q) if q is not None else None, m,
                                             radius, _fptr(out)))
        return out

    def getFluxAtPoints(self, points, normals=None, radius=None, dataIdx=0, norm=None, numNeighbors=0):
        """getFluxTensor(dataIdx, norm, numNeighbors) mapped to the query points as mapToPoints maps values, without the
        flux leaving the device (vr_get_flux_at_points_device); works after apply(collect=False).  Tensors in: a tensor
        out on the current torch stream.  Host arrays in: they are uploaded, and a numpy array comes back."""
        dev, p, q, m, ld, radius = self._mapArgs("getFluxAtPoints", points, normals, radius)
        import torch
        tdev = torch.device("cuda", self._device)
        if not dev:
            p = torch.from_numpy(p).to(tdev)
            q = None if q is None else torch.from_numpy(q).to(tdev)
        out = torch.empty(m, dtype=torch.float32, device=tdev)
        self._check(self._L.vr_get_flux_at_points_device(
            self._h, int(dataIdx), capi.VR_NORM_NONE if norm is None else int(norm), int(numNeighbors),
            C.c_void_p(p.data_ptr()), C.c_void_p(q.data_ptr()) if q is not None else None, m, ld, radius,
            C.c_void_p(out.data_ptr()), C.c_void_p(self._torch_stream())))
        return out if dev else out.cpu().numpy()

    # --- closest-hit queries for the caller's rays (vr_cast_rays*, include/viennaray_amd.h has the definition) ---------
    def castRays(self, origins, directions, tmax=float("inf"), followBoundaries=True, tnear=1e-4, returnPoints=False,
                 returnBoundaryHits=False):
        """Where does each ray hit?  m rays against the resident scene, traced as apply() traces a ray: the closest
        primitive, and with followBoundaries the side walls reflect, wrap or let through as the boundary conditions say,
        up to setMaxBoundaryHits walls.  Returns (prim, dist[, points][, boundaryHits]):
          prim  int32: the primitive's index, capi.VR_CAST_MISS (-1: left the scene, passed an IGNORE wall, or further
                than tmax) or capi.VR_CAST_WALL (-2: stopped on a wall — followBoundaries off, or the budget ran out);
          dist  float32: the path length, the float32 sum of the segments' t; +inf for a miss;
          points  [m, 3] float32 (returnPoints): where the ray ended; NaN for a miss;
          boundaryHits  int32 (returnBoundaryHits): the walls the ray was continued at.
        Directions are used as given, not normalised (on a 2-D tracer a z component is dropped first, and the direction
        is then normalised): dist and tmax are in units of the direction's length.  tnear applies to the first segment.
        float32 contiguous torch tensors on the tracer's device in ([m, 3]; [m, 2] on a 2-D tracer) give tensors out,
        computed on the device and ordered on the current torch stream (vr_cast_rays_device; any other tensor raises
        ValueError); host arrays in give numpy arrays out (vr_cast_rays).  Needs what apply() or applyPrepare() leaves
        behind for the geometry, boundary conditions and source direction in force, and changes none of it."""
        flags = capi.VR_CAST_FOLLOW_BOUNDARIES if followBoundaries else 0
        if hasattr(origins, "data_ptr") or hasattr(directions, "data_ptr"):
            import torch
            cols = [(None, 2), (None, 3)] if self.D == 2 else [(None, 3)]
            _check_device_tensor("castRays", "origins", origins, self._device, "torch.float32", cols)
            _check_device_tensor("castRays", "directions", directions, self._device, "torch.float32",
                                 [tuple(origins.shape)])
            m, ld = int(origins.shape[0]), int(origins.shape[1])
            dev = origins.device
            prim = torch.empty(m, dtype=torch.int32, device=dev)
            dist = torch.empty(m, dtype=torch.float32, device=dev)
            pts = torch.empty((m, 3), dtype=torch.float32, device=dev) if returnPoints else None
            bh = torch.empty(m, dtype=torch.int32, device=dev) if returnBoundaryHits else None
            self._check(self._L.vr_cast_rays_device(
                self._h, C.c_void_p(origins.data_ptr()), C.c_void_p(directions.data_ptr()), m, ld, float(tnear),
                float(tmax), flags, C.c_void_p(prim.data_ptr()), C.c_void_p(dist.data_ptr()),
                C.c_void_p(pts.data_ptr()) if pts is not None else None,
                C.c_void_p(bh.data_ptr()) if bh is not None else None, C.c_void_p(self._torch_stream())))
        else:
            o = np.asarray(origins, dtype=np.float32)
            o = o.reshape(-1, o.shape[-1]) if o.ndim == 2 else o.reshape(-1, 3)
            d = np.asarray(directions, dtype=np.float32).reshape(o.shape)
            if o.shape[1] == 2:  # 2-D rows: z := 0, as setGeometry does
                o = np.concatenate([o, np.zeros((o.shape[0], 1), np.float32)], axis=1)
                d = np.concatenate([d, np.zeros((d.shape[0], 1), np.float32)], axis=1)
            o, d = np.ascontiguousarray(o), np.ascontiguousarray(d)
            m = int(o.shape[0])
            prim = np.empty(m, dtype=np.int32)
            dist = np.empty(m, dtype=np.float32)
            pts = np.empty((m, 3), dtype=np.float32) if returnPoints else None
            bh = np.empty(m, dtype=np.uint32) if returnBoundaryHits else None
            self._check(self._L.vr_cast_rays(
                self._h, _fptr(o), _fptr(d), m, float(tnear), float(tmax), flags,
                prim.ctypes.data_as(C.POINTER(C.c_int32)), _fptr(dist), _fptr(pts) if pts is not None else None,
                bh.ctypes.data_as(C.POINTER(C.c_uint32)) if bh is not None else None))
            bh = bh.view(np.int32) if bh is not None else None
        return tuple(x for x in (prim, dist, pts, bh) if x is not None)

    def occluded(self, origins, targets):
        """Is there a primitive on the straight segment from origins[i] to targets[i]?  One boolean per row.  A cast
        along the unnormalised direction target - origin with tmax = 1 and the walls not followed: t runs in units of
        that direction's length, so t <= 1 is the segment (a primitive exactly at the target counts).  On a 2-D tracer the
        z components are left out.  Tensors in, a tensor out; host arrays in, a numpy array out."""
        if hasattr(origins, "data_ptr") or hasattr(targets, "data_ptr"):
            cols = [(None, 2), (None, 3)] if self.D == 2 else [(None, 3)]
            _check_device_tensor("occluded", "origins", origins, self._device, "torch.float32", cols)
            _check_device_tensor("occluded", "targets", targets, self._device, "torch.float32", [tuple(origins.shape)])
            o, d = origins, targets - origins
            if self.D == 2 and o.shape[1] == 3:
                o, d = o[:, :2].contiguous(), d[:, :2].contiguous()
        else:
            o = np.asarray(origins, dtype=np.float32)
            o = o.reshape(-1, o.shape[-1]) if o.ndim == 2 else o.reshape(-1, 3)
            d = np.asarray(targets, dtype=np.float32).reshape(o.shape) - o
            if self.D == 2:
                o, d = o[:, :2], d[:, :2]
        prim, _ = self.castRays(o, d, tmax=1.0, followBoundaries=False)
        return prim >= 0

    # --- gather flux: per-primitive direct flux by rays cast from the surface (vr_gather_flux*) -----------------------
    def gatherFlux(self, samples, cosinePower=1.0, mode=GatherMode.NORMAL, emission=None, primFirst=0, primCount=None,
                   numpy=False):
        """The flux each primitive receives straight from the source, estimated by `samples` rays cast from the primitive
        into its own hemisphere: one float32 per primitive of the range [primFirst, primFirst + primCount) (None: to the
        last primitive), SOURCE-normalised — an unoccluded primitive facing the source is 1, exactly so for
        cosinePower 1.  Every primitive gets the same number of samples whatever its depth.
          mode      GatherMode.NORMAL: samples follow the cosine law about the primitive's normal (any cosinePower >= 1);
                    GatherMode.SOURCE: they follow the source's power-cosine law (cosinePower >= 2, no emission).
          emission  one float per primitive of the scene: what a sample that lands on the FRONT of primitive j brings back
                    (incoming flux x reflectivity, in the same units) — one radiosity iteration.  None: such samples are 0.
        A pure function of scene, setRngSeed and arguments, with the same bits for any split of the range over calls.
        A float32 torch tensor on the tracer's device as emission gives a tensor out, on the current torch stream
        (vr_gather_flux_device); a host array gives a numpy array (vr_gather_flux); with no emission a tensor on the
        tracer's device comes back unless numpy=True.  Needs what apply() or applyPrepare() leaves behind for the
        geometry, boundary conditions and source direction in force, and changes none of it
        (include/viennaray_amd.h has the definition)."""
        n = int(self._L.vr_num_primitives(self._h))
        primFirst = int(primFirst)
        primCount = max(0, n - primFirst) if primCount is None else int(primCount)
        if primFirst < 0 or primCount < 0 or int(samples) < 0:
            raise ValueError("gatherFlux: samples, primFirst and primCount must not be negative")
        host = numpy if emission is None else not hasattr(emission, "data_ptr")
        if host:
            e = None
            if emission is not None:
                e = np.ascontiguousarray(emission, dtype=np.float32).reshape(-1)
                if e.size != n:
                    raise ValueError("gatherFlux: emission has %d entries, the scene %d primitives" % (e.size, n))
            out = np.empty(primCount, dtype=np.float32)
            self._check(self._L.vr_gather_flux(self._h, primFirst, primCount, int(samples), float(cosinePower), int(mode),
                                               _fptr(e) if e is not None else None, _fptr(out)))
            return out
        import torch
        dev = torch.device("cuda", self._device)
        if emission is not None:
            _check_device_tensor("gatherFlux", "emission", emission, self._device, "torch.float32", [(n,)])
        out = torch.empty(primCount, dtype=torch.float32, device=dev)
        self._check(self._L.vr_gather_flux_device(
            self._h, primFirst, primCount, int(samples), float(cosinePower), int(mode),
            C.c_void_p(emission.data_ptr()) if emission is not None else None, C.c_void_p(out.data_ptr()),
            C.c_void_p(self._torch_stream())))
        return out

    def debugGatherSamples(self, prim, first, count, mode=GatherMode.NORMAL, cosinePower=1.0):
        """(origin[3], normal[3], directions[count, 3]) of samples first .. first + count - 1 of primitive `prim`, as
        gatherFlux builds them (vr_debug_gather_samples)"""
        o, m = np.empty(3, np.float32), np.empty(3, np.float32)
        d = np.empty((int(count), 3), np.float32)
        self._check(self._L.vr_debug_gather_samples(self._h, int(prim), int(first), int(count), int(mode), float(cosinePower),
                                                    _fptr(o), _fptr(m), _fptr(d)))
        return o, m, d

    # --- path gather: multi-bounce flux by paths traced back from the surface (vr_gather_paths*) ---------------------
    def _pathReflectivity(self, name, sticking, reflectivity, host_only=False):
        """(device?, scalar, table) of exactly one of sticking / reflectivity: a scalar, a numpy array or a float32 tensor
        on the tracer's device, one value per primitive; reflectivity = 1 - sticking in float32"""
        if (sticking is None) == (reflectivity is None):
            raise ValueError("%s: give exactly one of sticking and reflectivity" % name)
        n = int(self._L.vr_num_primitives(self._h))
        given = sticking if reflectivity is None else reflectivity
        if hasattr(given, "data_ptr"):
            _check_device_tensor(name, "sticking" if reflectivity is None else "reflectivity", given, self._device,
                                 "torch.float32", [(n,)])
            table = ((1.0 - given) if reflectivity is None else given).contiguous()
            return (True, 0.0, table) if not host_only else (False, 0.0, table.cpu().numpy())
        if np.ndim(given) == 0:
            return False, (float(np.float32(1.0) - np.float32(given)) if reflectivity is None else float(given)), None
        table = np.ascontiguousarray(given, dtype=np.float32).reshape(-1)
        if table.size != n:
            raise ValueError("%s: the table has %d entries, the scene %d primitives" % (name, table.size, n))
        if reflectivity is None:
            table = (np.float32(1.0) - table).astype(np.float32)
        return False, 0.0, table

    def gatherPaths(self, samples, sticking=None, reflectivity=None, reflection=GatherReflection.SPECULAR, maxBounces=64,
                    cosinePower=1.0, primFirst=0, primCount=None, numpy=False):
        """The multi-bounce incoming flux of a species that is reflected with probability 1 - sticking, by gatherFlux's
        samples followed BACK through their reflections until they reach the source plane: one float32 per primitive of
        the range, SOURCE-normalised, the same number of samples at every depth.
          sticking | reflectivity  exactly one of them: a scalar, a numpy array or a float32 tensor on the tracer's device,
                                   one value per primitive, in [0, 1]; reflectivity = 1 - sticking.
          reflection               GatherReflection.SPECULAR: the mirror direction at every vertex (what a
                                   SpecularParticle does); GatherReflection.DIFFUSE: the cosine law about the normal hit
                                   (the steady state solveRadiosity iterates to, without a link table).
          maxBounces               reflections a path may make; the estimate lacks at most reflectivity^(maxBounces + 1).
                                   0 gives gatherFlux(samples) bit for bit.
        A pure function of scene, setRngSeed and arguments, with the same bits for any split of the range over calls.
        A tensor in gives a tensor out on torch's current stream (vr_gather_paths_device), a numpy array in a numpy array
        (vr_gather_paths); with a scalar a tensor comes back unless numpy=True.  Needs what apply() or applyPrepare()
        leaves behind, like gatherFlux, and changes none of it (include/viennaray_amd.h has the definition)."""
        n = int(self._L.vr_num_primitives(self._h))
        primFirst = int(primFirst)
        primCount = max(0, n - primFirst) if primCount is None else int(primCount)
        if primFirst < 0 or primCount < 0 or int(samples) < 0 or int(maxBounces) < 0:
            raise ValueError("gatherPaths: samples, maxBounces, primFirst and primCount must not be negative")
        device, scalar, table = self._pathReflectivity("gatherPaths", sticking, reflectivity)
        if not device and (table is not None or numpy):
            out = np.empty(primCount, dtype=np.float32)
            self._check(self._L.vr_gather_paths(self._h, primFirst, primCount, int(samples), float(cosinePower),
                                                int(reflection), int(maxBounces), _fptr(table) if table is not None else None,
                                                scalar, _fptr(out)))
            return out
        import torch
        out = torch.empty(primCount, dtype=torch.float32, device=torch.device("cuda", self._device))
        self._check(self._L.vr_gather_paths_device(
            self._h, primFirst, primCount, int(samples), float(cosinePower), int(reflection), int(maxBounces),
            C.c_void_p(table.data_ptr()) if device else None, scalar, C.c_void_p(out.data_ptr()),
            C.c_void_p(self._torch_stream())))
        return out

    def debugGatherPath(self, prim, sample, sticking=None, reflectivity=None, reflection=GatherReflection.SPECULAR,
                        maxBounces=64, cosinePower=1.0, maxVertices=None):
        """ONE path of gatherPaths — sample `sample` of primitive `prim` — as a dict (vr_debug_gather_path):
          ids [v] int64, points / arriving / normals / leaving [v, 3] float32: the stored vertices, vertex 0 the starting
                 primitive (arriving NaN), every later one a geometry hit (leaving NaN where the path ends on it);
          numVertices: all vertices of the path (maxVertices, default maxBounces + 2, caps the stored ones);
          end: capi.VR_GATHER_END_*; direction [3]: the final direction; throughput; weight (unquantised)."""
        _, scalar, table = self._pathReflectivity("debugGatherPath", sticking, reflectivity, host_only=True)
        cap = int(maxBounces) + 2 if maxVertices is None else int(maxVertices)
        ids = np.zeros(cap, dtype=np.uint32)
        data = np.full((cap, 4, 3), np.nan, dtype=np.float32)
        count, end = C.c_uint32(0), C.c_uint32(0)
        final = np.empty(3, np.float32)
        T, w = C.c_float(0.0), C.c_float(0.0)
        self._check(self._L.vr_debug_gather_path(
            self._h, int(prim), int(sample), float(cosinePower), int(reflection), int(maxBounces),
            _fptr(table) if table is not None else None, scalar, cap, ids.ctypes.data_as(C.POINTER(C.c_uint32)), _fptr(data),
            C.byref(count), C.byref(end), _fptr(final), C.byref(T), C.byref(w)))
        v = min(cap, int(count.value))
        return {"ids": ids[:v].astype(np.int64), "points": data[:v, 0], "arriving": data[:v, 1], "normals": data[:v, 2],
                "leaving": data[:v, 3], "numVertices": int(count.value), "end": int(end.value), "direction": final,
                "throughput": np.float32(T.value), "weight": np.float32(w.value)}

    # --- gather to a target error: sums, standard error, adaptive sample counts (vr_gather_sums*, vr_gather_adaptive*) --
    def _gatherRange(self, name, primFirst, primCount, *counts):
        n = int(self._L.vr_num_primitives(self._h))
        primFirst = int(primFirst)
        primCount = max(0, n - primFirst) if primCount is None else int(primCount)
        if primFirst < 0 or primCount < 0 or any(int(v) < 0 for v in counts):
            raise ValueError("%s: counts, primFirst and primCount must not be negative" % name)
        return n, primFirst, primCount

    def _fluxSpec(self, name, n, cosinePower, mode, emission, numpy):
        """(spec, host?, what the spec points to) of a gatherFlux sample"""
        spec = GatherSpecPOD(cosinePower=float(cosinePower), mode=int(mode), paths=0)
        host = numpy if emission is None else not hasattr(emission, "data_ptr")
        keep = None
        if emission is not None and host:
            keep = np.ascontiguousarray(emission, dtype=np.float32).reshape(-1)
            if keep.size != n:
                raise ValueError("%s: emission has %d entries, the scene %d primitives" % (name, keep.size, n))
            spec.emission = keep.ctypes.data
        elif emission is not None:
            _check_device_tensor(name, "emission", emission, self._device, "torch.float32", [(n,)])
            keep = emission
            spec.emission = emission.data_ptr()
        return spec, host, keep

    def _pathsSpec(self, name, sticking, reflectivity, reflection, maxBounces, cosinePower, numpy):
        """(spec, host?, what the spec points to) of a gatherPaths sample"""
        device, scalar, table = self._pathReflectivity(name, sticking, reflectivity)
        spec = GatherSpecPOD(cosinePower=float(cosinePower), mode=int(GatherMode.NORMAL), paths=1, reflection=int(reflection),
                             maxBounces=int(maxBounces), reflectivityScalar=scalar)
        if table is not None:
            spec.reflectivity = table.data_ptr() if device else table.ctypes.data
        return spec, (not device and (table is not None or numpy)), table

    def _gatherSums(self, spec, host, primFirst, primCount, chunkFirst, chunks, budget, laws=None, energy=None):
        """laws: None (vr_gather_sums*) or a GatherLawsPOD (vr_gather_angular_sums*); with it energy: None or a
        GatherEnergyPOD (vr_gather_energy_sums*)"""
        head = (self._h, C.byref(spec)) + ((C.byref(laws),) if laws is not None else ())
        head += (C.byref(energy),) if energy is not None else ()
        if host:
            s1, s2 = np.empty(primCount, dtype=np.int64), np.empty(primCount, dtype=np.int64)
            i64 = C.POINTER(C.c_int64)
            call = self._L.vr_gather_sums if laws is None else self._L.vr_gather_angular_sums
            call = call if energy is None else self._L.vr_gather_energy_sums
            self._check(call(*head, primFirst, primCount, int(chunkFirst), int(chunks), int(budget), s1.ctypes.data_as(i64),
                             s2.ctypes.data_as(i64)))
            return s1, s2
        import torch
        dev = torch.device("cuda", self._device)
        s1, s2 = torch.empty(primCount, dtype=torch.int64, device=dev), torch.empty(primCount, dtype=torch.int64, device=dev)
        call = self._L.vr_gather_sums_device if laws is None else self._L.vr_gather_angular_sums_device
        call = call if energy is None else self._L.vr_gather_energy_sums_device
        self._check(call(*head, primFirst, primCount, int(chunkFirst), int(chunks), int(budget), C.c_void_p(s1.data_ptr()),
                         C.c_void_p(s2.data_ptr()), C.c_void_p(self._torch_stream())))
        return s1, s2

    def _gatherAdaptive(self, spec, host, primFirst, primCount, target, absTarget, minSamples, maxSamples, returnInfo,
                        laws=None, energy=None):
        """laws: None (vr_gather_adaptive*) or a GatherLawsPOD (vr_gather_angular_adaptive*); with it energy: None or a
        GatherEnergyPOD (vr_gather_energy_adaptive*)"""
        info = GatherAdaptiveInfoPOD()
        head = (self._h, C.byref(spec)) + ((C.byref(laws),) if laws is not None else ())
        head += (C.byref(energy),) if energy is not None else ()
        if host:
            flux, err = np.empty(primCount, dtype=np.float32), np.empty(primCount, dtype=np.float32)
            used = np.empty(primCount, dtype=np.uint32)
            call = self._L.vr_gather_adaptive if laws is None else self._L.vr_gather_angular_adaptive
            call = call if energy is None else self._L.vr_gather_energy_adaptive
            self._check(call(*head, primFirst, primCount, int(minSamples), int(maxSamples), float(target), float(absTarget),
                             _fptr(flux), _fptr(err), used.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(info)))
        else:
            import torch
            dev = torch.device("cuda", self._device)
            flux, err = torch.empty(primCount, dtype=torch.float32, device=dev), torch.empty(primCount, dtype=torch.float32, device=dev)
            store = torch.empty(primCount, dtype=torch.int32, device=dev)  # (the uint32 counts, at most 2^22)
            call = self._L.vr_gather_adaptive_device if laws is None else self._L.vr_gather_angular_adaptive_device
            call = call if energy is None else self._L.vr_gather_energy_adaptive_device
            self._check(call(*head, primFirst, primCount, int(minSamples), int(maxSamples), float(target), float(absTarget),
                             C.c_void_p(flux.data_ptr()), C.c_void_p(err.data_ptr()), C.c_void_p(store.data_ptr()), C.byref(info),
                             C.c_void_p(self._torch_stream())))
            used = store
        return (flux, err, used, info.as_dict()) if returnInfo else (flux, err, used)

    def gatherFluxAdaptive(self, target, minSamples=64, maxSamples=4096, absTarget=0.0, cosinePower=1.0, mode=GatherMode.NORMAL,
                           emission=None, primFirst=0, primCount=None, returnInfo=False, numpy=False):
        """gatherFlux to a target error: every primitive starts with minSamples samples (a multiple of 64) and doubles its
        own count until the standard error of its mean is at most max(target x mean, absTarget) or maxSamples
        (minSamples times a power of two) is reached.  Returns (flux, stdErr, samples): float32, float32 and the sample
        count used, one per primitive of the range; with returnInfo a dict {rounds, unconverged, totalSamples} as well.
        flux[i] has the bits of gatherFlux(samples[i]) wherever no weight exceeds 2^22 / maxSamples (every NORMAL
        weight).  target = absTarget = 0 runs every primitive to maxSamples.  A primitive whose first minSamples samples
        all weigh 0 stops there with flux 0 and stdErr 0: the call cannot know better.  A pure function of scene,
        setRngSeed and arguments; tensors and numpy arrays as gatherFlux (vr_gather_adaptive*)."""
        n, primFirst, primCount = self._gatherRange("gatherFluxAdaptive", primFirst, primCount, minSamples, maxSamples)
        spec, host, keep = self._fluxSpec("gatherFluxAdaptive", n, cosinePower, mode, emission, numpy)
        return self._gatherAdaptive(spec, host, primFirst, primCount, target, absTarget, minSamples, maxSamples, returnInfo)

    def gatherPathsAdaptive(self, target, sticking=None, reflectivity=None, reflection=GatherReflection.SPECULAR, maxBounces=64,
                            minSamples=64, maxSamples=4096, absTarget=0.0, cosinePower=1.0, primFirst=0, primCount=None,
                            returnInfo=False, numpy=False):
        """gatherPaths to a target error, as gatherFluxAdaptive: (flux, stdErr, samples), plus the info dict when asked;
        sticking | reflectivity, reflection and maxBounces as gatherPaths, tensors and numpy arrays likewise."""
        _, primFirst, primCount = self._gatherRange("gatherPathsAdaptive", primFirst, primCount, minSamples, maxSamples, maxBounces)
        spec, host, keep = self._pathsSpec("gatherPathsAdaptive", sticking, reflectivity, reflection, maxBounces, cosinePower, numpy)
        return self._gatherAdaptive(spec, host, primFirst, primCount, target, absTarget, minSamples, maxSamples, returnInfo)

    def gatherFluxSums(self, chunkFirst, chunks, budget, cosinePower=1.0, mode=GatherMode.NORMAL, emission=None, primFirst=0,
                       primCount=None, numpy=False):
        """(sum, sumSq): per primitive of the range the exact int64 sums of gatherFlux's quantised weights (2^-40) and of
        their squares (2^-28) over samples [64 chunkFirst, 64 (chunkFirst + chunks)) of a call of `budget` samples.
        float32(sum / 2^40 / K) over chunks [0, K / 64) with budget K has the bits of gatherFlux(K); sums over adjacent
        chunk ranges add (vr_gather_sums*)."""
        n, primFirst, primCount = self._gatherRange("gatherFluxSums", primFirst, primCount, chunkFirst, chunks, budget)
        spec, host, keep = self._fluxSpec("gatherFluxSums", n, cosinePower, mode, emission, numpy)
        return self._gatherSums(spec, host, primFirst, primCount, chunkFirst, chunks, budget)

    def gatherPathsSums(self, chunkFirst, chunks, budget, sticking=None, reflectivity=None, reflection=GatherReflection.SPECULAR,
                        maxBounces=64, cosinePower=1.0, primFirst=0, primCount=None, numpy=False):
        """(sum, sumSq) as gatherFluxSums, of gatherPaths's samples"""
        _, primFirst, primCount = self._gatherRange("gatherPathsSums", primFirst, primCount, chunkFirst, chunks, budget, maxBounces)
        spec, host, keep = self._pathsSpec("gatherPathsSums", sticking, reflectivity, reflection, maxBounces, cosinePower, numpy)
        return self._gatherSums(spec, host, primFirst, primCount, chunkFirst, chunks, budget)

    # --- angular gather: a path weighed by tabulated source radiance, sticking and yield (vr_gather_angular*) --------
    def _angularLaws(self, name, sourceLaw, reflectivityLaw, yieldLaw, stickingLaw=None):
        """(GatherLawsPOD, the host arrays it points to): each law None or 2 .. 256 values over a cosine in [0, 1], a
        sequence, a numpy array or a tensor (the tables are always handed over as HOST arrays); stickingLaw is accepted
        in place of reflectivityLaw as 1 - R in float32"""
        if stickingLaw is not None:
            if reflectivityLaw is not None:
                raise ValueError("%s: give at most one of stickingLaw and reflectivityLaw" % name)
            t = stickingLaw.detach().cpu().numpy() if hasattr(stickingLaw, "data_ptr") else stickingLaw
            reflectivityLaw = (np.float32(1.0) - np.asarray(t, dtype=np.float32)).astype(np.float32)
        pod, keep = GatherLawsPOD(), []
        for field, count, law in (("sourceLaw", "sourceCount", sourceLaw), ("reflectivityLaw", "reflectivityCount", reflectivityLaw),
                                  ("yieldLaw", "yieldCount", yieldLaw)):
            if law is None:
                continue
            if hasattr(law, "data_ptr"):
                law = law.detach().cpu().numpy()
            t = np.ascontiguousarray(law, dtype=np.float32).reshape(-1)
            keep.append(t)
            setattr(pod, field, t.ctypes.data)
            setattr(pod, count, t.size)
        return pod, keep

    def gatherAngular(self, samples, sourceLaw=None, reflectivityLaw=None, yieldLaw=None, sticking=None, reflectivity=None,
                      reflection=GatherReflection.SPECULAR, maxBounces=64, primFirst=0, primCount=None, numpy=False,
                      cosinePower=1.0, stickingLaw=None):
        """gatherPaths with up to three tabulated ANGULAR LAWS: each 2 .. 256 float32 values read as the piecewise-linear
        function of a cosine in [0, 1], nodes at k / (M - 1).
          sourceLaw        L(c), the source's radiance by c = u . direction relative to a Lambertian source (a measured
                           sputter-target distribution; c^(n - 1) is the power cosine).  Normalised by the library; needs
                           cosinePower == 1.  The law weighs the samples, it does not place them.
          reflectivityLaw  R(mu), the share NOT absorbed at a vertex by mu = normal . leaving direction, the forward
                           particle's cosine of incidence; the throughput takes (T * reflectivity) * R(mu).  stickingLaw=
                           is accepted as 1 - R.
          yieldLaw         Y(mu0) by the sample's initial direction against the starting primitive's normal: the etch or
                           resputter yield of what arrives; it may exceed 1.
        sticking | reflectivity, reflection, maxBounces, the range, tensors and numpy arrays as gatherPaths (the laws
        themselves are always read on the host).  With no law, or with all-ones laws, the result has gatherPaths's bits
        (vr_gather_angular*; include/viennaray_amd.h has the definition)."""
        _, primFirst, primCount = self._gatherRange("gatherAngular", primFirst, primCount, samples, maxBounces)
        spec, host, keep = self._pathsSpec("gatherAngular", sticking, reflectivity, reflection, maxBounces, cosinePower, numpy)
        laws, keepLaws = self._angularLaws("gatherAngular", sourceLaw, reflectivityLaw, yieldLaw, stickingLaw)
        if host:
            out = np.empty(primCount, dtype=np.float32)
            self._check(self._L.vr_gather_angular(self._h, C.byref(spec), C.byref(laws), primFirst, primCount, int(samples),
                                                  _fptr(out)))
            return out
        import torch
        out = torch.empty(primCount, dtype=torch.float32, device=torch.device("cuda", self._device))
        self._check(self._L.vr_gather_angular_device(self._h, C.byref(spec), C.byref(laws), primFirst, primCount, int(samples),
                                                     C.c_void_p(out.data_ptr()), C.c_void_p(self._torch_stream())))
        return out

    def gatherAngularAdaptive(self, target, sourceLaw=None, reflectivityLaw=None, yieldLaw=None, sticking=None, reflectivity=None,
                              reflection=GatherReflection.SPECULAR, maxBounces=64, minSamples=64, maxSamples=4096, absTarget=0.0,
                              primFirst=0, primCount=None, returnInfo=False, numpy=False, cosinePower=1.0, stickingLaw=None):
        """gatherAngular to a target error, as gatherPathsAdaptive: (flux, stdErr, samples), plus the info dict when asked;
        flux[i] has the bits of gatherAngular(samples[i]) (vr_gather_angular_adaptive*)."""
        _, primFirst, primCount = self._gatherRange("gatherAngularAdaptive", primFirst, primCount, minSamples, maxSamples, maxBounces)
        spec, host, keep = self._pathsSpec("gatherAngularAdaptive", sticking, reflectivity, reflection, maxBounces, cosinePower, numpy)
        laws, keepLaws = self._angularLaws("gatherAngularAdaptive", sourceLaw, reflectivityLaw, yieldLaw, stickingLaw)
        return self._gatherAdaptive(spec, host, primFirst, primCount, target, absTarget, minSamples, maxSamples, returnInfo, laws)

    def gatherAngularSums(self, chunkFirst, chunks, budget, sourceLaw=None, reflectivityLaw=None, yieldLaw=None, sticking=None,
                          reflectivity=None, reflection=GatherReflection.SPECULAR, maxBounces=64, primFirst=0, primCount=None,
                          numpy=False, cosinePower=1.0, stickingLaw=None):
        """(sum, sumSq) as gatherPathsSums, of gatherAngular's samples (vr_gather_angular_sums*)"""
        _, primFirst, primCount = self._gatherRange("gatherAngularSums", primFirst, primCount, chunkFirst, chunks, budget, maxBounces)
        spec, host, keep = self._pathsSpec("gatherAngularSums", sticking, reflectivity, reflection, maxBounces, cosinePower, numpy)
        laws, keepLaws = self._angularLaws("gatherAngularSums", sourceLaw, reflectivityLaw, yieldLaw, stickingLaw)
        return self._gatherSums(spec, host, primFirst, primCount, chunkFirst, chunks, budget, laws)

    def debugGatherAngularPath(self, prim, sample, laws=None, sticking=None, reflectivity=None, reflection=GatherReflection.SPECULAR,
                               maxBounces=64, cosinePower=1.0, maxVertices=None):
        """ONE path of gatherAngular, as debugGatherPath's dict.  laws: None or a dict with any of the keys sourceLaw,
        reflectivityLaw, stickingLaw, yieldLaw.  Every vertex's mu is normals[v] . leaving[v]; throughput and weight are
        the path's under the laws (vr_debug_gather_angular_path)."""
        _, scalar, table = self._pathReflectivity("debugGatherAngularPath", sticking, reflectivity, host_only=True)
        spec = GatherSpecPOD(cosinePower=float(cosinePower), mode=int(GatherMode.NORMAL), paths=1, reflection=int(reflection),
                             maxBounces=int(maxBounces), reflectivityScalar=scalar)
        if table is not None:
            spec.reflectivity = table.ctypes.data
        laws = dict(laws or {})
        unknown = set(laws) - {"sourceLaw", "reflectivityLaw", "stickingLaw", "yieldLaw"}
        if unknown:
            raise ValueError("debugGatherAngularPath: unknown laws %s" % sorted(unknown))
        pod, keepLaws = self._angularLaws("debugGatherAngularPath", laws.get("sourceLaw"), laws.get("reflectivityLaw"),
                                          laws.get("yieldLaw"), laws.get("stickingLaw"))
        cap = int(maxBounces) + 2 if maxVertices is None else int(maxVertices)
        ids = np.zeros(cap, dtype=np.uint32)
        data = np.full((cap, 4, 3), np.nan, dtype=np.float32)
        count, end = C.c_uint32(0), C.c_uint32(0)
        final = np.empty(3, np.float32)
        T, w = C.c_float(0.0), C.c_float(0.0)
        self._check(self._L.vr_debug_gather_angular_path(
            self._h, C.byref(spec), C.byref(pod), int(prim), int(sample), cap, ids.ctypes.data_as(C.POINTER(C.c_uint32)),
            _fptr(data), C.byref(count), C.byref(end), _fptr(final), C.byref(T), C.byref(w)))
        v = min(cap, int(count.value))
        return {"ids": ids[:v].astype(np.int64), "points": data[:v, 0], "arriving": data[:v, 1], "normals": data[:v, 2],
                "leaving": data[:v, 3], "numVertices": int(count.value), "end": int(end.value), "direction": final,
                "throughput": np.float32(T.value), "weight": np.float32(w.value)}

    # --- energy gather: an ion's energy lost along a path, a yield by the arrival energy (vr_gather_energy*) ----------
    def _energyTables(self, name, energyYield, energyMax, sourceEnergy, sourceQuantiles, retentionLaw, energyCut):
        """(GatherEnergyPOD, the host arrays it points to): energyYield 2 .. 256 values over e = E / energyMax in [0, 1];
        sourceQuantiles None or 2 .. 256 values of the source's inverse CDF over u in [0, 1]; retentionLaw None or 2 .. 256
        values over a cosine in [0, 1].  Sequences, numpy arrays or tensors, always handed over as HOST arrays"""
        if energyYield is None or energyMax is None:
            raise ValueError("%s: energyYield and energyMax are required" % name)
        if sourceEnergy is not None and sourceQuantiles is not None:
            raise ValueError("%s: give at most one of sourceEnergy and sourceQuantiles" % name)
        if sourceEnergy is None and sourceQuantiles is None:
            raise ValueError("%s: give sourceEnergy (a monoenergetic source) or sourceQuantiles" % name)
        pod, keep = GatherEnergyPOD(), []
        for field, count, law in (("energyYield", "energyYieldCount", energyYield),
                                  ("sourceQuantiles", "sourceQuantilesCount", sourceQuantiles),
                                  ("retentionLaw", "retentionCount", retentionLaw)):
            if law is None:
                continue
            if hasattr(law, "data_ptr"):
                law = law.detach().cpu().numpy()
            t = np.ascontiguousarray(law, dtype=np.float32).reshape(-1)
            keep.append(t)
            setattr(pod, field, t.ctypes.data)
            setattr(pod, count, t.size)
        pod.energyMax = float(energyMax)
        pod.sourceEnergy = float(sourceEnergy) if sourceEnergy is not None else 0.0
        pod.energyCut = int(energyCut)
        return pod, keep

    def gatherEnergy(self, samples, energyYield=None, energyMax=None, sourceEnergy=None, sourceQuantiles=None, retentionLaw=None,
                     energyCut=True, sourceLaw=None, reflectivityLaw=None, yieldLaw=None, sticking=None, reflectivity=None,
                     reflection=GatherReflection.SPECULAR, maxBounces=64, primFirst=0, primCount=None, numpy=False,
                     cosinePower=1.0, stickingLaw=None):
        """gatherAngular with the ion's ENERGY carried along every path: the ion leaves the source with E0, keeps the share
        retentionLaw(mu) of its energy at every reflection, and the path's weight takes one more multiply, by
        energyYield(E / energyMax) of the energy it arrives with.
          energyYield      Y_E(e), 2 .. 256 values over e = E / energyMax in [0, 1] (sqrt(E) - sqrt(E_th), 0 below the
                           threshold, tabulated); required, as energyMax.
          sourceEnergy     the one energy of a monoenergetic source, or
          sourceQuantiles  the source's inverse CDF Q(u), 2 .. 256 values over u in [0, 1]: E0 = Q(u), u a counter draw
                           of (seed, primitive, sample).
          retentionLaw     eps(mu) in [0, 1] by mu = normal . leaving direction, reflectivityLaw's mu; None: no loss.
          energyCut        end a path (GatherEnd.ENERGY) as soon as its energy has entered the leading zeros of
                           energyYield: it can only weigh 0.  No bit of the result depends on it.
        Everything else as gatherAngular.  With an all-ones energyYield the result has gatherAngular's bits
        (vr_gather_energy*; include/viennaray_amd.h has the definition)."""
        _, primFirst, primCount = self._gatherRange("gatherEnergy", primFirst, primCount, samples, maxBounces)
        spec, host, keep = self._pathsSpec("gatherEnergy", sticking, reflectivity, reflection, maxBounces, cosinePower, numpy)
        laws, keepLaws = self._angularLaws("gatherEnergy", sourceLaw, reflectivityLaw, yieldLaw, stickingLaw)
        energy, keepEnergy = self._energyTables("gatherEnergy", energyYield, energyMax, sourceEnergy, sourceQuantiles, retentionLaw,
                                                energyCut)
        if host:
            out = np.empty(primCount, dtype=np.float32)
            self._check(self._L.vr_gather_energy(self._h, C.byref(spec), C.byref(laws), C.byref(energy), primFirst, primCount,
                                                 int(samples), _fptr(out)))
            return out
        import torch
        out = torch.empty(primCount, dtype=torch.float32, device=torch.device("cuda", self._device))
        self._check(self._L.vr_gather_energy_device(self._h, C.byref(spec), C.byref(laws), C.byref(energy), primFirst, primCount,
                                                    int(samples), C.c_void_p(out.data_ptr()), C.c_void_p(self._torch_stream())))
        return out

    def gatherEnergyAdaptive(self, target, energyYield=None, energyMax=None, sourceEnergy=None, sourceQuantiles=None,
                             retentionLaw=None, energyCut=True, sourceLaw=None, reflectivityLaw=None, yieldLaw=None, sticking=None,
                             reflectivity=None, reflection=GatherReflection.SPECULAR, maxBounces=64, minSamples=64,
                             maxSamples=4096, absTarget=0.0, primFirst=0, primCount=None, returnInfo=False, numpy=False,
                             cosinePower=1.0, stickingLaw=None):
        """gatherEnergy to a target error, as gatherAngularAdaptive: (flux, stdErr, samples), plus the info dict when
        asked; flux[i] has the bits of gatherEnergy(samples[i]) (vr_gather_energy_adaptive*)."""
        _, primFirst, primCount = self._gatherRange("gatherEnergyAdaptive", primFirst, primCount, minSamples, maxSamples, maxBounces)
        spec, host, keep = self._pathsSpec("gatherEnergyAdaptive", sticking, reflectivity, reflection, maxBounces, cosinePower, numpy)
        laws, keepLaws = self._angularLaws("gatherEnergyAdaptive", sourceLaw, reflectivityLaw, yieldLaw, stickingLaw)
        energy, keepEnergy = self._energyTables("gatherEnergyAdaptive", energyYield, energyMax, sourceEnergy, sourceQuantiles,
                                                retentionLaw, energyCut)
        return self._gatherAdaptive(spec, host, primFirst, primCount, target, absTarget, minSamples, maxSamples, returnInfo, laws,
                                    energy)

    def gatherEnergySums(self, chunkFirst, chunks, budget, energyYield=None, energyMax=None, sourceEnergy=None,
                         sourceQuantiles=None, retentionLaw=None, energyCut=True, sourceLaw=None, reflectivityLaw=None,
                         yieldLaw=None, sticking=None, reflectivity=None, reflection=GatherReflection.SPECULAR, maxBounces=64,
                         primFirst=0, primCount=None, numpy=False, cosinePower=1.0, stickingLaw=None):
        """(sum, sumSq) as gatherAngularSums, of gatherEnergy's samples (vr_gather_energy_sums*)"""
        _, primFirst, primCount = self._gatherRange("gatherEnergySums", primFirst, primCount, chunkFirst, chunks, budget, maxBounces)
        spec, host, keep = self._pathsSpec("gatherEnergySums", sticking, reflectivity, reflection, maxBounces, cosinePower, numpy)
        laws, keepLaws = self._angularLaws("gatherEnergySums", sourceLaw, reflectivityLaw, yieldLaw, stickingLaw)
        energy, keepEnergy = self._energyTables("gatherEnergySums", energyYield, energyMax, sourceEnergy, sourceQuantiles,
                                                retentionLaw, energyCut)
        return self._gatherSums(spec, host, primFirst, primCount, chunkFirst, chunks, budget, laws, energy)

    _ENERGY_KEYS = {"energyYield", "energyMax", "sourceEnergy", "sourceQuantiles", "retentionLaw", "energyCut"}

    def debugGatherEnergyPath(self, prim, sample, energy, laws=None, sticking=None, reflectivity=None,
                              reflection=GatherReflection.SPECULAR, maxBounces=64, cosinePower=1.0, maxVertices=None):
        """ONE path of gatherEnergy, as debugGatherAngularPath's dict plus "u", "E0", "P" and "e": the energy draw, the
        energy at the source, the product of the retentions and the arrival energy in table units.  energy: a dict with
        gatherEnergy's keywords energyYield, energyMax, sourceEnergy | sourceQuantiles, retentionLaw, energyCut; laws as
        debugGatherAngularPath.  "end" is a GatherEnd; a sample the cut ended before its walk has numVertices == 1
        (vr_debug_gather_energy_path)."""
        _, scalar, table = self._pathReflectivity("debugGatherEnergyPath", sticking, reflectivity, host_only=True)
        spec = GatherSpecPOD(cosinePower=float(cosinePower), mode=int(GatherMode.NORMAL), paths=1, reflection=int(reflection),
                             maxBounces=int(maxBounces), reflectivityScalar=scalar)
        if table is not None:
            spec.reflectivity = table.ctypes.data
        laws, energy = dict(laws or {}), dict(energy or {})
        unknown = set(laws) - {"sourceLaw", "reflectivityLaw", "stickingLaw", "yieldLaw"}
        if unknown:
            raise ValueError("debugGatherEnergyPath: unknown laws %s" % sorted(unknown))
        unknown = set(energy) - self._ENERGY_KEYS
        if unknown:
            raise ValueError("debugGatherEnergyPath: unknown energy keys %s" % sorted(unknown))
        pod, keepLaws = self._angularLaws("debugGatherEnergyPath", laws.get("sourceLaw"), laws.get("reflectivityLaw"),
                                          laws.get("yieldLaw"), laws.get("stickingLaw"))
        epod, keepEnergy = self._energyTables("debugGatherEnergyPath", energy.get("energyYield"), energy.get("energyMax"),
                                              energy.get("sourceEnergy"), energy.get("sourceQuantiles"), energy.get("retentionLaw"),
                                              energy.get("energyCut", True))
        cap = int(maxBounces) + 2 if maxVertices is None else int(maxVertices)
        ids = np.zeros(cap, dtype=np.uint32)
        data = np.full((cap, 4, 3), np.nan, dtype=np.float32)
        count, end = C.c_uint32(0), C.c_uint32(0)
        final, e4 = np.empty(3, np.float32), np.zeros(4, np.float32)
        T, w = C.c_float(0.0), C.c_float(0.0)
        self._check(self._L.vr_debug_gather_energy_path(
            self._h, C.byref(spec), C.byref(pod), C.byref(epod), int(prim), int(sample), cap,
            ids.ctypes.data_as(C.POINTER(C.c_uint32)), _fptr(data), C.byref(count), C.byref(end), _fptr(final), C.byref(T),
            C.byref(w), _fptr(e4)))
        v = min(cap, int(count.value))
        return {"ids": ids[:v].astype(np.int64), "points": data[:v, 0], "arriving": data[:v, 1], "normals": data[:v, 2],
                "leaving": data[:v, 3], "numVertices": int(count.value), "end": int(end.value), "direction": final,
                "throughput": np.float32(T.value), "weight": np.float32(w.value), "u": e4[0], "E0": e4[1], "P": e4[2],
                "e": e4[3]}

    # --- species gather: several species weighed along one set of traced paths (vr_gather_species*) ------------------
    _SPECIES_KEYS = {"sticking", "reflectivity", "cosinePower", "sourceLaw", "reflectivityLaw", "stickingLaw", "yieldLaw"}

    def _speciesSpecs(self, name, species, reflection, maxBounces, numpy):
        """(specs array, laws array, host?, what they point to) of a list of species dicts"""
        species = list(species)
        specs, laws, keep = (GatherSpecPOD * max(1, len(species)))(), (GatherLawsPOD * max(1, len(species)))(), []
        forms = set()
        for s, sp in enumerate(species):
            sp = dict(sp)
            unknown = set(sp) - self._SPECIES_KEYS
            if unknown:
                raise ValueError("%s: species %d: unknown keys %s" % (name, s, sorted(unknown)))
            who = "%s: species %d" % (name, s)
            device, scalar, table = self._pathReflectivity(who, sp.get("sticking"), sp.get("reflectivity"))
            specs[s] = GatherSpecPOD(cosinePower=float(sp.get("cosinePower", 1.0)), mode=int(GatherMode.NORMAL), paths=1,
                                     reflection=int(reflection), maxBounces=int(maxBounces), reflectivityScalar=scalar)
            if table is not None:
                specs[s].reflectivity = table.data_ptr() if device else table.ctypes.data
                forms.add("device" if device else "host")
            laws[s], keepLaws = self._angularLaws(who, sp.get("sourceLaw"), sp.get("reflectivityLaw"), sp.get("yieldLaw"),
                                                  sp.get("stickingLaw"))
            keep += [table, keepLaws]
        if len(forms) > 1:
            raise ValueError("%s: the species' tables are tensors (the device form) or numpy arrays (the host form), not both" % name)
        host = "host" in forms or (not forms and numpy)
        return specs, laws, len(species), host, keep

    def gatherSpecies(self, samples, species, reflection=GatherReflection.SPECULAR, maxBounces=64, primFirst=0, primCount=None,
                      numpy=False):
        """gatherAngular for up to capi.VR_GATHER_MAX_SPECIES species along ONE set of traced paths: [S, primCount] float32,
        row s with the bits of gatherAngular called with species s's arguments.  A path's geometry does not depend on the
        species; what differs is each one's multiplies along it, so S species cost about the walk of the one that lives
        longest.
          species  a list of dicts with keys from sticking | reflectivity (exactly one: a scalar, a numpy array or a
                   float32 tensor on the tracer's device, per primitive), cosinePower, sourceLaw, reflectivityLaw |
                   stickingLaw, yieldLaw — gatherAngular's arguments of those names.  Unknown keys raise ValueError.
          reflection, maxBounces  shared by all species: they make the path.
        Tensor tables select the device form (a tensor out, on torch's current stream), numpy tables the host form;
        mixing the two raises ValueError; with scalars alone a tensor comes back unless numpy=True
        (vr_gather_species*; include/viennaray_amd.h has the definition)."""
        _, primFirst, primCount = self._gatherRange("gatherSpecies", primFirst, primCount, samples, maxBounces)
        specs, laws, S, host, keep = self._speciesSpecs("gatherSpecies", species, reflection, maxBounces, numpy)
        if host:
            out = np.empty((S, primCount), dtype=np.float32)
            self._check(self._L.vr_gather_species(self._h, specs, laws, S, primFirst, primCount, int(samples), _fptr(out)))
            return out
        import torch
        out = torch.empty((S, primCount), dtype=torch.float32, device=torch.device("cuda", self._device))
        self._check(self._L.vr_gather_species_device(self._h, specs, laws, S, primFirst, primCount, int(samples),
                                                     C.c_void_p(out.data_ptr()), C.c_void_p(self._torch_stream())))
        return out

    def gatherSpeciesSums(self, chunkFirst, chunks, budget, species, reflection=GatherReflection.SPECULAR, maxBounces=64,
                          primFirst=0, primCount=None, numpy=False):
        """(sum, sumSq), two int64 [S, primCount]: row s as gatherAngularSums gives them for species s, along one set of
        traced paths; species, reflection, maxBounces, tensors and numpy arrays as gatherSpecies (vr_gather_species_sums*)"""
        _, primFirst, primCount = self._gatherRange("gatherSpeciesSums", primFirst, primCount, chunkFirst, chunks, budget, maxBounces)
        specs, laws, S, host, keep = self._speciesSpecs("gatherSpeciesSums", species, reflection, maxBounces, numpy)
        if host:
            s1, s2 = np.empty((S, primCount), dtype=np.int64), np.empty((S, primCount), dtype=np.int64)
            i64 = C.POINTER(C.c_int64)
            self._check(self._L.vr_gather_species_sums(self._h, specs, laws, S, primFirst, primCount, int(chunkFirst), int(chunks),
                                                       int(budget), s1.ctypes.data_as(i64), s2.ctypes.data_as(i64)))
            return s1, s2
        import torch
        dev = torch.device("cuda", self._device)
        s1, s2 = torch.empty((S, primCount), dtype=torch.int64, device=dev), torch.empty((S, primCount), dtype=torch.int64, device=dev)
        self._check(self._L.vr_gather_species_sums_device(self._h, specs, laws, S, primFirst, primCount, int(chunkFirst), int(chunks),
                                                          int(budget), C.c_void_p(s1.data_ptr()), C.c_void_p(s2.data_ptr()),
                                                          C.c_void_p(self._torch_stream())))
        return s1, s2

    def gatherSpeciesAdaptive(self, target, species, reflection=GatherReflection.SPECULAR, maxBounces=64, minSamples=64,
                              maxSamples=4096, absTarget=0.0, primFirst=0, primCount=None, returnInfo=False, numpy=False):
        """gatherSpecies to a target error per species: (flux, stdErr, samples), each [S, primCount], row s with the bits
        of gatherAngularAdaptive called with species s's arguments and targets.  The rounds are gatherPathsAdaptive's,
        run once for all species along one set of traced paths; on every primitive each species stops at its own K, and
        one that has stopped no longer keeps the shared path going.
          target, absTarget  a scalar, which applies to all species, or a sequence of S values
          species, reflection, maxBounces, tensors and numpy arrays  as gatherSpecies
          minSamples, maxSamples  as gatherPathsAdaptive
        With returnInfo a dict as well: rounds, unconverged (a list of S), totalSamples (a list of S: what each species'
        own call reports) and walkedSamples, the samples actually walked — per primitive the largest count among its
        species (vr_gather_species_adaptive*; include/viennaray_amd.h has the definition)."""
        _, primFirst, primCount = self._gatherRange("gatherSpeciesAdaptive", primFirst, primCount, minSamples, maxSamples, maxBounces)
        specs, laws, S, host, keep = self._speciesSpecs("gatherSpeciesAdaptive", species, reflection, maxBounces, numpy)

        def targets(what, value):
            t = np.asarray(value, dtype=np.float32).reshape(-1)
            if t.size == 1:
                t = np.repeat(t, max(1, S))
            if t.size != max(1, S):
                raise ValueError("gatherSpeciesAdaptive: %s takes a scalar or one value per species (%d), not %d" % (what, S, t.size))
            return np.ascontiguousarray(t)

        rel, absT = targets("target", target), targets("absTarget", absTarget)
        info = capi.GatherSpeciesAdaptiveInfoPOD()
        if host:
            flux, err = np.empty((S, primCount), dtype=np.float32), np.empty((S, primCount), dtype=np.float32)
            used = np.empty((S, primCount), dtype=np.uint32)
            self._check(self._L.vr_gather_species_adaptive(self._h, specs, laws, S, primFirst, primCount, int(minSamples), int(maxSamples),
                                                           _fptr(rel), _fptr(absT), _fptr(flux), _fptr(err),
                                                           used.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(info)))
        else:
            import torch
            dev = torch.device("cuda", self._device)
            flux = torch.empty((S, primCount), dtype=torch.float32, device=dev)
            err = torch.empty((S, primCount), dtype=torch.float32, device=dev)
            used = torch.empty((S, primCount), dtype=torch.int32, device=dev)  # (the uint32 counts, at most 2^22)
            self._check(self._L.vr_gather_species_adaptive_device(
                self._h, specs, laws, S, primFirst, primCount, int(minSamples), int(maxSamples), _fptr(rel), _fptr(absT),
                C.c_void_p(flux.data_ptr()), C.c_void_p(err.data_ptr()), C.c_void_p(used.data_ptr()), C.byref(info),
                C.c_void_p(self._torch_stream())))
        return (flux, err, used, info.as_dict(S)) if returnInfo else (flux, err, used)

    # --- radiosity solve: the steady-state flux of a diffusely re-emitting species (vr_radiosity_*) ------------------
    def radiosityLinkBytes(self, samples):
        """bytes of device memory the link table for `samples` samples per primitive takes (vr_radiosity_link_bytes)"""
        return int(self._L.vr_radiosity_link_bytes(self._h, int(samples)))

    def radiosityLinks(self, samples, cosinePower=1.0):
        """Build (or replace) the link table solveRadiosity iterates over: gatherFlux's samples walked once, the primitive
        each lands on recorded (vr_radiosity_links_device).  Needs what apply() or applyPrepare() leaves behind, like
        gatherFlux, and changes none of it.  On torch's current stream."""
        self._check(self._L.vr_radiosity_links_device(self._h, int(samples), float(cosinePower),
                                                      C.c_void_p(self._torch_stream())))

    def freeRadiosityLinks(self):
        """give the link table's memory back (vr_radiosity_free_links)"""
        self._check(self._L.vr_radiosity_free_links(self._h))

    def debugRadiosityLinks(self, prim, first, count):
        """links first .. first + count - 1 of primitive `prim` in the resident table, as original ids; -1: the sample
        brings nothing back from the surface (vr_debug_radiosity_links)"""
        out = np.empty(int(count), dtype=np.int32)
        self._check(self._L.vr_debug_radiosity_links(self._h, int(prim), int(first), int(count),
                                                     out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def solveRadiosity(self, samples, sticking=None, reflectivity=None, cosinePower=1.0, tolerance=1e-4, maxIterations=1000,
                       returnInfo=False):
        """The steady-state incoming flux of a species that is re-emitted diffusely with probability 1 - sticking: the
        fixed point of gatherFlux(samples, emission=reflectivity * flux), one float32 per primitive, SOURCE-normalised.
          sticking | reflectivity  exactly one of them: a scalar, a numpy array or a float32 tensor on the tracer's device,
                                   one value per primitive, in [0, 1]; reflectivity = 1 - sticking.
          tolerance                the solve stops at the first iteration whose largest change of a flux value is at most
                                   this, or after maxIterations; maxIterations=0 gives gatherFlux(samples).
        The samples are walked once, into a link table that stays resident (radiosityLinkBytes(samples) bytes) and is
        reused while samples, cosinePower and the scene's settings stay as they are: several species share one table.
        A tensor in gives a tensor out on torch's current stream, anything else a numpy array.  returnInfo=True:
        (flux, iterations, residual).  A pure function of scene, setRngSeed and arguments (include/viennaray_amd.h has
        the definition)."""
        if (sticking is None) == (reflectivity is None):
            raise ValueError("solveRadiosity: give exactly one of sticking and reflectivity")
        n = int(self._L.vr_num_primitives(self._h))
        given = sticking if reflectivity is None else reflectivity
        device = hasattr(given, "data_ptr")
        scalar, table = 0.0, None
        if device:
            _check_device_tensor("solveRadiosity", "sticking" if reflectivity is None else "reflectivity", given,
                                 self._device, "torch.float32", [(n,)])
            table = (1.0 - given) if reflectivity is None else given
            table = table.contiguous()
        elif np.ndim(given) == 0:
            scalar = float(np.float32(1.0) - np.float32(given)) if reflectivity is None else float(given)
        else:
            table = np.ascontiguousarray(given, dtype=np.float32).reshape(-1)
            if table.size != n:
                raise ValueError("solveRadiosity: the table has %d entries, the scene %d primitives" % (table.size, n))
            if reflectivity is None:
                table = (np.float32(1.0) - table).astype(np.float32)
        if not self._L.vr_radiosity_resident(self._h, int(samples), float(cosinePower)):
            self.radiosityLinks(samples, cosinePower)
        its, res = C.c_uint32(0), C.c_float(0.0)
        if device:
            import torch
            out = torch.empty(n, dtype=torch.float32, device=torch.device("cuda", self._device))
            self._check(self._L.vr_radiosity_solve_device(
                self._h, C.c_void_p(table.data_ptr()), 0.0, float(tolerance), int(maxIterations),
                C.c_void_p(out.data_ptr()), C.byref(its), C.byref(res), C.c_void_p(self._torch_stream())))
        else:
            out = np.empty(n, dtype=np.float32)
            self._check(self._L.vr_radiosity_solve(self._h, _fptr(table) if table is not None else None, scalar,
                                                   float(tolerance), int(maxIterations), _fptr(out), C.byref(its),
                                                   C.byref(res)))
        return (out, int(its.value), float(res.value)) if returnInfo else out

    # --- flux statistics: per-primitive hit counts and the Monte-Carlo error of the flux --------------------------
    def setCalculateFluxError(self, on=True):
        """Keep two more sums per primitive and particle alongside the flux label (vr_set_flux_statistics): the number of
        credits and the sum of their squares.  Off by default.  A per-credit estimator: it ignores the correlation
        between several credits of one ray to the same primitive."""
        self._check(self._L.vr_set_flux_statistics(self._h, int(bool(on))))
        self._fluxStats = bool(on)

    def numAccumulatorPlanes(self):
        """planes of numPrims int64 the accumulator array holds (fluxAccumulators / bindFluxAccumulators): the data labels
        of all particles and, with flux statistics on, two more behind each particle's labels"""
        parts = max(1, len(getattr(self, "_particles", None) or [None]))
        return max(1, self.numData()) + (2 * parts if getattr(self, "_fluxStats", False) else 0)

    def getHitCounts(self, particleIdx=0):
        """credits to the flux label of every primitive in the last apply (uint64)"""
        out = np.empty(self._n, dtype=np.uint64)
        self._check(self._L.vr_get_hit_counts(self._h, int(particleIdx), C.c_void_p(out.ctypes.data), self._n))
        return out

    def getFluxSumSquares(self, particleIdx=0):
        """sum over those credits of the squared credited value (float64, exact: acc / 2^40)"""
        out = np.empty(self._n, dtype=np.float64)
        self._check(self._L.vr_get_flux_sum_squares(self._h, int(particleIdx), C.c_void_p(out.ctypes.data), self._n))
        return out

    def _fluxError(self, particleIdx, kind):
        out = np.empty(self._n, dtype=np.float32)
        self._check(self._L.vr_get_flux_error(self._h, int(particleIdx), int(kind), C.c_void_p(out.ctypes.data), self._n))
        return out

    def getFluxRelativeError(self, particleIdx=0):
        """sigma / S1 per primitive, +inf where nothing was credited; the same for every NormalizationType"""
        return self._fluxError(particleIdx, 0)

    def getFluxAbsoluteError(self, particleIdx=0):
        """sigma = sqrt(max(sumsq - S1^2 / N, 0)) per primitive, in raw flux units (N: the rays of the whole apply)"""
        return self._fluxError(particleIdx, 1)

    def getFluxErrorTensor(self, particleIdx=0, kind="relative"):
        """The relative or absolute error as a new torch.float32 tensor on the tracer's device, computed and left there
        (vr_get_flux_error_device), ordered on the current torch stream; works after apply(collect=False)."""
        import torch
        if kind not in ("relative", "absolute"):
            raise ValueError("getFluxErrorTensor: kind is 'relative' or 'absolute'")
        dev = torch.device("cuda", self._device)
        out = torch.empty(self._n, dtype=torch.float32, device=dev)
        self._check(self._L.vr_get_flux_error_device(self._h, int(particleIdx), 0 if kind == "relative" else 1,
                                                     C.c_void_p(out.data_ptr()), self._n,
                                                     C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        return out

    def getFluxErrorDevice(self, particleIdx=0, kind="relative"):
        """the façade's name for getFluxErrorTensor"""
        return self.getFluxErrorTensor(particleIdx, kind)

    def raysForRelativeError(self, target, quantile=0.95, particleIdx=0):
        """The ray count at which the `quantile` of the finite relative errors of the last apply would reach `target`:
        ceil(N * (q / target)^2), N the rays of that apply (the error falls with 1 / sqrt(N))."""
        if not target > 0:
            raise ValueError("raysForRelativeError: target must be positive")
        rel = self.getFluxRelativeError(particleIdx)
        rel = rel[np.isfinite(rel)]
        if rel.size == 0:
            raise VrError("raysForRelativeError: no primitive received any flux in the last apply")
        q = float(np.quantile(rel.astype(np.float64), float(quantile)))
        return int(math.ceil(float(self.getRayTraceInfo().numRays) * (q / float(target)) ** 2))

    def smoothFlux(self, flux, numNeighbors=1):
        f = np.ascontiguousarray(flux, dtype=np.float32).copy()
        self._check(self._L.vr_smooth_flux(self._h, _fptr(f), f.size, int(numNeighbors)))
        return f

    # --- geometry-derived values -----------------------------------------------
    def getBoundingBox(self):
        out = np.empty(6, dtype=np.float32)
        self._check(self._L.vr_get_bounding_box(self._h, _fptr(out)))
        return out.reshape(2, 3)

    def getSourceArea(self):
        return self._L.vr_get_source_area(self._h)

    def fluxAccumulators(self):
        """(device pointer, n) of the int64 fixed-point accumulators."""
        p = C.c_void_p()
        n = C.c_uint32()
        self._check(self._L.vr_flux_accumulators(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    # --- the data log (DataLog / logData, rayTraceKernel.hpp:131-133, 345) --------
    def setDataLogShape(self, rowSizes):
        """Entries per row of the data log the log_data hook of a stateful model fills (at most 16 rows, 65536 entries
        in all); an empty list clears the shape and nothing is logged."""
        a = np.ascontiguousarray(rowSizes, dtype=np.uint32).reshape(-1)
        self._check(self._L.vr_set_data_log_shape(self._h, a.ctypes.data_as(C.POINTER(C.c_uint32)), a.size))
        self._logRows = [int(v) for v in a]

    def _log_rows(self, flat):
        out, o = [], 0
        for n in getattr(self, "_logRows", []):
            out.append(flat[o:o + n].copy())
            o += n
        return out

    def getDataLog(self):
        """The last apply's log: one float32 array per row."""
        flat = np.empty(sum(getattr(self, "_logRows", [])), dtype=np.float32)
        self._check(self._L.vr_get_data_log(self._h, _fptr(flat), flat.size))
        return self._log_rows(flat)

    def dataLogAccumulators(self):
        """The last apply's int64 fixed-point sums (value * 2^24), rows concatenated."""
        flat = np.empty(sum(getattr(self, "_logRows", [])), dtype=np.int64)
        self._check(self._L.vr_get_data_log_i64(self._h, flat.ctypes.data_as(C.POINTER(C.c_int64)), flat.size))
        return flat

    def getDataLogDropped(self):
        """log calls of the last apply that were dropped: outside the shape, or a negative / non-finite / too large value"""
        v = C.c_uint64(0)
        self._check(self._L.vr_get_data_log_dropped(self._h, C.byref(v)))
        return int(v.value)

    def dataLogDevice(self):
        """(device pointer, n) of the int64 sums for a caller's own collective; the dropped counter and the overflow flag
        are the two words behind them (vr_data_log_accumulators)."""
        p = C.c_void_p()
        n = C.c_uint32()
        self._check(self._L.vr_data_log_accumulators(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def bindFluxAccumulators(self, dev_ptr, n):
        """Use a caller-owned device buffer of n int64 (e.g. a torch tensor)."""
        self._check(self._L.vr_bind_flux_accumulators(self._h, C.c_void_p(dev_ptr), int(n)))

    # --- diagnostics ---------------------------------------------------------------
    def debugIntersect(self, org, dirn, tnear=1e-4):
        o = np.ascontiguousarray(org, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirn, dtype=np.float32).reshape(-1, 3)
        n = o.shape[0]
        tn = np.full(n, tnear, dtype=np.float32)
        g = np.empty(n, dtype=np.int32)
        p = np.empty(n, dtype=np.uint32)
        t = np.empty(n, dtype=np.float32)
        self._check(self._L.vr_debug_intersect(self._h, _fptr(o), _fptr(d), _fptr(tn), n,
                                               g.ctypes.data_as(C.POINTER(C.c_int32)),
                                               p.ctypes.data_as(C.POINTER(C.c_uint32)), _fptr(t)))
        return g, p, t

    def debugProcessHit(self, org, dirn, tfar, primID):
        """Boundary::processHit on the device: (new origins, new directions, reflect flags)"""
        o = np.ascontiguousarray(org, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirn, dtype=np.float32).reshape(-1, 3)
        n = o.shape[0]
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(tfar, dtype=np.float32), (n,)))
        p = np.ascontiguousarray(np.broadcast_to(np.asarray(primID, dtype=np.uint32), (n,)))
        oo, do = np.empty_like(o), np.empty_like(d)
        r = np.empty(n, dtype=np.int32)
        self._check(self._L.vr_debug_process_hit(self._h, _fptr(o), _fptr(d), _fptr(t),
                                                 p.ctypes.data_as(C.POINTER(C.c_uint32)), n, _fptr(oo), _fptr(do),
                                                 r.ctypes.data_as(C.POINTER(C.c_int32))))
        return oo, do, r.astype(bool)

    def debugModelSourceSample(self, idx, seed):
        """the active stateful model's generator (init, then the source sample): first origin, direction and the engine
        outputs consumed before the trace, per global ray index"""
        i = np.ascontiguousarray(idx, dtype=np.uint64)
        o = np.empty((i.size, 3), dtype=np.float32)
        d = np.empty((i.size, 3), dtype=np.float32)
        k = np.empty(i.size, dtype=np.uint32)
        self._check(self._L.vr_debug_model_source_sample(self._h, i.ctypes.data_as(C.POINTER(C.c_uint64)), i.size,
                                                         int(seed), _fptr(o), _fptr(d),
                                                         k.ctypes.data_as(C.POINTER(C.c_uint32))))
        return o, d, k

    def debugSurfaceSourceSample(self, idx, seed):
        """the surface source's sample of global ray indices idx for kernel seed `seed`, by the generator's own device
        function: origin, direction, start weight, engine outputs consumed"""
        i = np.ascontiguousarray(idx, dtype=np.uint64)
        o = np.empty((i.size, 3), dtype=np.float32)
        d = np.empty((i.size, 3), dtype=np.float32)
        w = np.empty(i.size, dtype=np.float32)
        k = np.empty(i.size, dtype=np.uint32)
        self._check(self._L.vr_debug_surface_source_sample(self._h, i.ctypes.data_as(C.POINTER(C.c_uint64)), i.size,
                                                           int(seed), _fptr(o), _fptr(d), _fptr(w),
                                                           k.ctypes.data_as(C.POINTER(C.c_uint32))))
        return o, d, w, k

    def debugUserSourceSample(self, idx, seed):
        """the sample of the source model in force for global ray indices idx and kernel seed `seed`, by the generator's
        own device function: origin, direction, start weight, engine outputs consumed"""
        i = np.ascontiguousarray(idx, dtype=np.uint64)
        o = np.empty((i.size, 3), dtype=np.float32)
        d = np.empty((i.size, 3), dtype=np.float32)
        w = np.empty(i.size, dtype=np.float32)
        k = np.empty(i.size, dtype=np.uint32)
        self._check(self._L.vr_debug_user_source_sample(self._h, i.ctypes.data_as(C.POINTER(C.c_uint64)), i.size,
                                                        int(seed), _fptr(o), _fptr(d), _fptr(w),
                                                        k.ctypes.data_as(C.POINTER(C.c_uint32))))
        return o, d, w, k

    def debugSourceSample(self, idx, seed):
        i = np.ascontiguousarray(idx, dtype=np.uint64)
        o = np.empty((i.size, 3), dtype=np.float32)
        d = np.empty((i.size, 3), dtype=np.float32)
        self._check(self._L.vr_debug_source_sample(self._h, i.ctypes.data_as(C.POINTER(C.c_uint64)), i.size,
                                                   int(seed), _fptr(o), _fptr(d)))
        return o, d

    def debugRngOutputs(self, idx, seed, count):
        out = np.empty(count, dtype=np.uint64)
        self._check(self._L.vr_debug_rng_outputs(self._h, int(idx), int(seed), count,
                                                 out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out

    def debugIssueRate(self, kind, waves_per_simd, iters=20000):
        """Measured issue ceiling: dict(rate [counted instr/s], clock_hz, seconds, count)."""
        out = (C.c_double * 4)()
        self._check(self._L.vr_debug_issue_rate(self._h, int(kind), int(waves_per_simd), int(iters), out))
        return dict(rate=out[0], clock_hz=out[1], seconds=out[2], count=out[3])

    def debugBvhCheck(self):
        v = C.c_uint32(0)
        self._check(self._L.vr_debug_bvh_check(self._h, C.byref(v)))
        return int(v.value)

    def debugBvhStats(self):
        a = (C.c_uint32 * 3)()
        self._check(self._L.vr_debug_bvh_stats(self._h, a))
        return dict(nodes=a[0], leaves=a[1], maxDepth=a[2])


class TraceDisk(Trace):
    """rayTraceDisk.hpp:13-224"""

    def setGeometry(self, points, normals, gridDelta, diskRadius=0.0):
        """points / normals: [n, 2] or [n, 3].  Two torch tensors on the context's device (float32, contiguous) are
        handed over where they are (vr_set_disks_device): the library copies them on the device, ordered behind the
        current torch stream, and the tensors may be overwritten as soon as this returns.  A tensor on a device that
        cannot go that way raises ValueError — it is never copied through the host behind the caller's back."""
        if _on_any_device(points) or _on_any_device(normals):
            return self._setGeometryDevice(points, normals, gridDelta, diskRadius)
        p = np.ascontiguousarray(points, dtype=np.float32)
        n = np.ascontiguousarray(normals, dtype=np.float32)
        if p.shape[1] == 2:  # 2-D points: z := 0 (rayGeometryDisk.hpp:148-151)
            p = np.concatenate([p, np.zeros((p.shape[0], 1), np.float32)], axis=1)
            n = np.concatenate([n, np.zeros((n.shape[0], 1), np.float32)], axis=1)
        p = np.ascontiguousarray(p)
        n = np.ascontiguousarray(n)
        assert p.shape == n.shape, "Geometry: Points/Normals size mismatch"
        self._n = p.shape[0]
        self._check(self._L.vr_set_disks(self._h, _fptr(p), _fptr(n), self._n, float(gridDelta),
                                         float(diskRadius), self.D))
        self._gridDelta = float(gridDelta)

    def _setGeometryDevice(self, points, normals, gridDelta, diskRadius):
        # (two columns need D == 2: refused as a shape, where the shape is looked at)
        cols = [(None, 2), (None, 3)] if self.D == 2 else [(None, 3)]
        _check_device_tensor("setGeometry", "points", points, self._device, "torch.float32", cols)
        _check_device_tensor("setGeometry", "normals", normals, self._device, "torch.float32", cols)
        if tuple(points.shape) != tuple(normals.shape):
            raise ValueError(f"setGeometry: shape: points {tuple(points.shape)} and normals {tuple(normals.shape)} differ")
        n, ld = int(points.shape[0]), int(points.shape[1])
        self._check(self._L.vr_set_disks_device(self._h, C.c_void_p(points.data_ptr()), C.c_void_p(normals.data_ptr()),
                                                n, ld, float(gridDelta), float(diskRadius), self.D,
                                                C.c_void_p(self._torch_stream())))
        self._n = n
        self._gridDelta = float(gridDelta)

    def getDiskAreas(self):
        out = np.empty(self._n, dtype=np.float32)
        self._check(self._L.vr_get_disk_areas(self._h, _fptr(out), self._n))
        return out

    def getDiskRadius(self):
        return self._L.vr_get_disk_radius(self._h)

    def getNeighborCounts(self):
        out = np.empty(self._n, dtype=np.uint32)
        self._check(self._L.vr_get_neighbor_counts(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32)), self._n))
        return out


class TraceTriangle(Trace):
    """rayTraceTriangle.hpp:13-154"""

    def setLineGeometry(self, nodes, lines, gridDelta):
        """setGeometry(LineMesh) (rayTraceTriangle.hpp:76-81, D == 2): lines -> triangle strips.  Host arrays only: the
        strips are made on the host (io.lines_to_triangles); a device-side LineMesh is out of scope — convert on the
        device and hand the triangles to setGeometry as tensors."""
        from . import io
        v, t, _ = io.lines_to_triangles(nodes, lines, gridDelta)
        self.setGeometry(v, t, gridDelta)

    def setGeometry(self, points, triangles, gridDelta):
        """points: [nv, 3], triangles: [nt, 3] vertex indices.  Two torch tensors on the tracer's device (points
        float32, triangles int32 — torch has no general uint32; a negative value reads as an index out of range and is
        refused — both contiguous) are handed over where they are (vr_set_triangles_device): validated and copied on
        the device, ordered behind the current torch stream, and the tensors may be overwritten as soon as this
        returns.  A tensor that cannot go that way raises ValueError — it is never copied through the host behind the
        caller's back."""
        if _on_any_device(points) or _on_any_device(triangles):
            return self._setGeometryDevice(points, triangles, gridDelta)
        v = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        t = np.ascontiguousarray(triangles, dtype=np.uint32).reshape(-1, 3)
        self._n = t.shape[0]
        self._check(self._L.vr_set_triangles(self._h, _fptr(v), v.shape[0],
                                             t.ctypes.data_as(C.POINTER(C.c_uint32)), self._n,
                                             float(gridDelta), self.D))
        self._gridDelta = float(gridDelta)

    def debugTriangleMesh(self):
        """(unit normals [nt, 3], areas [nt]) of the mesh in force (vr_debug_triangle_mesh)"""
        nrm = np.empty((self._n, 3), dtype=np.float32)
        area = np.empty(self._n, dtype=np.float32)
        self._check(self._L.vr_debug_triangle_mesh(self._h, _fptr(nrm), _fptr(area), self._n))
        return nrm, area

    def _setGeometryDevice(self, points, triangles, gridDelta):
        _check_device_tensor("setGeometry", "points", points, self._device, "torch.float32", [(None, 3)])
        _check_device_tensor("setGeometry", "triangles", triangles, self._device, "torch.int32", [(None, 3)])
        nv, nt = int(points.shape[0]), int(triangles.shape[0])
        self._check(self._L.vr_set_triangles_device(self._h, C.c_void_p(points.data_ptr()), nv,
                                                    C.c_void_p(triangles.data_ptr()), nt, float(gridDelta), self.D,
                                                    C.c_void_p(self._torch_stream())))
        self._n = nt
        self._gridDelta = float(gridDelta)
