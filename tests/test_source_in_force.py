"""One ray source in force (RaySource, viennaray_amd/csrc/vr_source.hpp): whichever source a tracer had before, after a
setter it traces exactly what a fresh tracer with that source traces, and each of the four clearing calls takes back what
its row of the clearing table says — no more, no less.  Bit-exact comparisons only (int64 accumulators, every TraceInfo
counter, the trace mode), on the stepped plane of tests/test_source_models.py: the smallest scene on which an absorbing
particle gets an absorbing kernel, which makes "no absorbing kernel under start weights" visible in traceMode().
"""
import ctypes as C

import numpy as np
import pytest

import viennaray_amd as vr
from viennaray_amd import capi
from test_source_models import F, RAYS, _model, _run, _same, _scene, _tracer, _use_cache, cache  # noqa: F401 (fixtures)

STATES = ("random", "tilted", "grid", "host", "host+weights", "surface", "beam", "rejection")
MODELS = ("beam", "rejection")
STICKINGS = (1.0, 0.1)
TILT = (0.2, 0.1, -1.0)
_, P, N = _scene(3)
GRID = vr.SourceGrid(P[:200] + np.array([0.0, 0.0, 6.0], F))
_rng = np.random.default_rng(20)
HOST_ORG = np.stack([_rng.uniform(0, 35, RAYS), _rng.uniform(0, 35, RAYS), np.full(RAYS, 6.0)], axis=1).astype(F)
_d = np.stack([_rng.uniform(-0.5, 0.5, RAYS), _rng.uniform(-0.5, 0.5, RAYS), np.full(RAYS, -1.0)], axis=1)
HOST_DIR = (_d / np.linalg.norm(_d, axis=1, keepdims=True)).astype(F)
HOST_DRAWS = np.full(RAYS, 4, np.uint32)
HOST_WEIGHTS = _rng.uniform(0.25, 1.25, RAYS).astype(F)
SURF_WEIGHTS = np.linspace(0.5, 1.5, 10).astype(F)


def _set(t, state, before=None):
    """put `state` in force on a tracer whose state was `before` (None: a fresh tracer)"""
    if before == "tilted" and state != "tilted":
        t._check(t._L.vr_set_primary_direction(t._h, None))  # (every state but "tilted" runs with it off)
    if state in ("random", "tilted"):
        t.resetSource()
        if state == "tilted":
            t.setPrimaryDirection(TILT)
    elif state == "grid":
        t.setSource(GRID)
    elif state == "host":
        t.setHostRays(HOST_ORG, HOST_DIR, HOST_DRAWS)
    elif state == "host+weights":
        t.setHostRays(HOST_ORG, HOST_DIR, HOST_DRAWS, weights=HOST_WEIGHTS)
    elif state == "surface":
        t.setSurfaceSource(P[:10], N[:10], SURF_WEIGHTS, 1.0, 1e-3)
    else:
        t.setSource(_model(state))


@pytest.fixture(scope="module")
def fresh(cache):
    """(sticking, state) -> the result of a fresh tracer with that source; computed once, never changed"""
    out = {}
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("VR_CACHE_DIR", cache)  # (module scope: the per-test fixture that sets it has not run yet)
        for sticking in STICKINGS:
            for state in STATES:
                t = _tracer(3, sticking, rays=RAYS)
                _set(t, state)
                out[(sticking, state)] = _run(t)
    return out


def _every_ordered_pair(n):
    """a cyclic sequence over range(n) in which every ordered pair, (k, k) included, is adjacent exactly once: the de Bruijn
    sequence B(n, 2) by the standard Lyndon-word construction"""
    a, seq = [0] * (2 * n), []

    def db(t, p):
        if t > 2:
            if 2 % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, n):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    return seq


def test_the_walk_contains_every_transition():
    seq = _every_ordered_pair(len(STATES))
    assert len(seq) == 64
    assert {(seq[k], seq[(k + 1) % 64]) for k in range(64)} == {(a, b) for a in range(8) for b in range(8)}


@pytest.mark.gpu
@pytest.mark.parametrize("sticking", STICKINGS)
def test_every_transition_equals_a_fresh_tracer(sticking, fresh, cache):
    """ONE tracer through all 64 ordered pairs of the eight states, each state also set twice in a row"""
    seq = [STATES[k] for k in _every_ordered_pair(len(STATES))]
    t = _tracer(3, sticking, rays=RAYS)
    _set(t, seq[0])
    before = seq[0]
    for state in seq[1:] + seq[:1]:
        _set(t, state, before)
        _same(_run(t), fresh[(sticking, state)], f"{before} -> {state}")
        before = state


@pytest.mark.gpu
@pytest.mark.parametrize("sticking", STICKINGS)
def test_the_eight_states_trace_differently(sticking, fresh):
    """no two states give the same accumulators: a walk that failed to switch sources would not pass by accident"""
    for a in range(len(STATES)):
        for b in range(a + 1, len(STATES)):
            assert not np.array_equal(fresh[(sticking, STATES[a])][0], fresh[(sticking, STATES[b])][0]), (STATES[a], STATES[b])


def _after_clearing(call, state):
    """the clearing table: the state in force after `call`, by the one before it.  ("tilted" is SourceRandom: no source
    setter touches the primary direction.)"""
    if state == "tilted":
        return state
    if call in ("resetSource", "setHostRays(empty)"):
        return "random"
    if call == "clearSurfaceSource":
        return "random" if state == "surface" else state
    assert call == "setSource(None)"
    return "random" if state in MODELS else state


CLEARING = {
    "resetSource": lambda t: t.resetSource(),
    "setHostRays(empty)": lambda t: t.setHostRays(np.zeros((0, 3), F), np.zeros((0, 3), F)),
    "clearSurfaceSource": lambda t: t.clearSurfaceSource(),
    "setSource(None)": lambda t: t.setSource(None),
}


@pytest.mark.gpu
@pytest.mark.parametrize("sticking", STICKINGS)
def test_clearing_calls_follow_the_table(sticking, fresh, cache):
    t = _tracer(3, sticking, rays=RAYS)
    before = None
    for state in STATES:
        for call, clear in CLEARING.items():
            _set(t, state, before)
            clear(t)
            after = _after_clearing(call, state)
            _same(_run(t), fresh[(sticking, after)], f"{state} -> {call}")
            before = after


@pytest.mark.gpu
def test_start_weights_rule_out_the_absorbing_kernels(fresh):
    """at sticking 1 host rays without weights run an absorbing kernel; with weights of their own, a surface source and a
    model with kHasWeight do not (fails if the scene ever stops selecting an absorbing kernel)"""
    host = fresh[(1.0, "host")][2]
    assert host in (1, 2), host
    assert fresh[(1.0, "beam")][2] in (1, 2)
    for state in ("host+weights", "surface", "rejection"):
        assert fresh[(1.0, state)][2] != host, (state, host)


@pytest.mark.gpu
@pytest.mark.parametrize("state", ["surface", "beam"])
def test_refused_host_ray_weights_leave_the_source_in_force(state, fresh, cache):
    """weights of the host rays' count, after another source took the host rays' place: refused, nothing changes"""
    t = _tracer(3, 0.1, rays=RAYS)
    _set(t, "host")
    _set(t, state, "host")
    rc = t._L.vr_set_host_ray_weights(t._h, HOST_WEIGHTS.ctypes.data_as(C.POINTER(C.c_float)), RAYS)
    assert rc == capi.VR_E_INVALID
    assert t._L.vr_last_error(t._h).decode() == "vr_set_host_ray_weights: one weight per host ray (call vr_set_host_rays first)"
    _same(_run(t), fresh[(0.1, state)], f"{state} after refused weights")
