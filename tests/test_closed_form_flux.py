"""The device against the closed forms of tests/closed_forms.py: the same scenes through the same builders, the same
cases, the same references and the same tolerance formulas as tests/test_closed_form_flux_host.py holds the oracle to,
evaluated at the device's ray count.  Nothing here is compared with the oracle (the rest of the suite does that): a law
that the oracle restated wrongly, and the device reproduced bit for bit, fails here on its own.

What separates the laws: the cos^n cases see the source's exponent alone; diffuse 1.0 the normalisation and the first
hit; diffuse 0.2 the diffuse reflection and the weight chain; specular 0.3 the specular law, the chain and the walls'
images; periodic x against reflective x (the same answer by symmetry) how a wall continues a ray; the disk clouds the
multi-disc crediting and the exposed-area normalisation.  The trace mode the tracer picked goes into every message;
forcing modes is not this file's job (bit-equality across modes is proved elsewhere).
"""
import numpy as np
import pytest

import viennaray_amd as vr
from viennaray_amd import BoundaryCondition as BC

import closed_forms as cf

pytestmark = pytest.mark.gpu

_BC = {cf.REFLECTIVE: BC.REFLECTIVE_BOUNDARY, cf.PERIODIC: BC.PERIODIC_BOUNDARY}


def tracer_of(case_id):
    case = cf.CASES[cf.CASE_IDS.index(case_id)]
    S = cf.scene_of(case_id)
    if S.kind == "mesh":
        t = vr.TraceTriangle(3)
        t.setGeometry(S.geom.verts, S.geom.tris, 1.0)
    else:
        t = vr.TraceDisk(S.D)
        t.setGeometry(S.geom.points, S.geom.normals, 1.0)
    t.setBoundaryConditions([_BC[b] for b in S.bcs])
    if S.source_direction is not None:
        t.setSourceDirection(S.source_direction)
    if case.particle == cf.DIFFUSE:
        t.setParticleType(vr.DiffuseParticle(case.sticking, "flux"))
    else:
        t.setParticleType(vr.SpecularParticle(case.sticking, case.power, "flux"))
    t.setRngSeed(cf.SEED)
    return t, S


@pytest.mark.parametrize("case_id", cf.CASE_IDS)
def test_device_matches_the_closed_form(case_id):
    t, S = tracer_of(case_id)
    t.setNumberOfRaysFixed(cf.GPU_RAYS)
    t.apply(collect=False)
    flux = t.getFluxNormalized()
    who = "device (trace mode %d)" % t.traceMode()
    assert abs(t.getSourceArea() - S.source_area) <= 1e-5 * S.source_area, who
    assert int(t.getRayTraceInfo().numRays) == cf.GPU_RAYS, who
    report, failures, worst = cf.compare(case_id, flux, cf.GPU_RAYS, who)
    print("\n" + "\n".join(report))
    assert not failures, "\n".join(failures)


SURFACE_AREA = 500.0      # deliberately not the emitting area (240): the constant below is then not 1
SURFACE_OFFSET = 1e-3
SURFACE_RAYS_PER_POINT = 41667    # 480 points: 2.0e7 rays


def test_surface_source_is_the_second_term_of_the_series():
    """setSurfaceSource has no oracle restatement; its reference is the second term of the Neumann series, K . W.

    Emit from the centroids of the n = 480 bottom and wall triangles of the mesh, along their normals, with weights
    W_j = F_direct(centroid j) and R rays each, sticking 1.  The constant between the tracer's SOURCE-normalised flux
    and K . W, from INTEGRATION.md section 3 (the surface-source row) and vr_results.cpp (normalize_on_device):

      raw flux of primitive t   = sum of the weights of the rays that end on t  ~  R sum_j W_j P(j -> t)
      normalizeFlux(SOURCE)     = raw * sourceArea / numRays / area(t),  numRays = n R,  sourceArea = the caller's
      mean over a row's 2 ny triangles of area 1/2
                                = sourceArea / (n R) * R sum_j W_j P(j -> row) / (2 ny * 1/2)
      P(j -> row)               = the 2-D view factor V(j -> cell): the row runs the whole periodic length in y
      K . W at the row          = sum over the 2 emitters q of each profile cell, each standing for a length 1/2,
                                  of W_q * 1/2 * V(q -> cell) / |cell|        (reciprocity, |cell| = 1)
      grouping the n emitters by profile position (ny at each): sum_j = ny sum_q, hence
      flux(row)                 = sourceArea / (n * 1/2) * (K . W)(row)  =  sourceArea / (emitting area) * (K . W)(row)

    So C = SURFACE_AREA / 240.  Two assertions: every row's ratio is C, and the ratio does not vary across rows.
    K . W is evaluated with the emitters where the tracer has them (points at 1/3 and 2/3 of each cell, not spread over
    the cell: that matters within a cell of a corner) and the receiving side on the reference's own segments.
    Tolerance: the rays carry unequal weights, so the binomial count is replaced by the effective one, E =
    (sum_q n_q R W_q V_q)^2 / sum_q n_q R W_q^2 V_q, from the reference alone; bound 5 / sqrt(E) + 2e-3 as elsewhere."""
    t, S = tracer_of("mesh-diffuse-1.0")
    mesh = S.geom
    R = cf.radiosity(cf.W, cf.DEPTH, 1.0)
    cen, nrm = cf.triangle_centroids(mesh)
    emit = np.nonzero(mesh.part != cf.TOP)[0]
    n = len(emit)
    assert n == 480
    pos = np.where(mesh.part[emit] == cf.BOTTOM, cen[emit, 0], cen[emit, 2])   # the emitter's profile coordinate
    W, _, _ = R.direct_at(mesh.part[emit], pos)
    t.setNumberOfRaysPerPoint(SURFACE_RAYS_PER_POINT)
    t.setSurfaceSource(cen[emit].astype(np.float32), nrm[emit].astype(np.float32), W.astype(np.float32),
                       SURFACE_AREA, SURFACE_OFFSET)
    t.apply(collect=False)
    flux = t.getFluxNormalized().astype(np.float64)
    who = "device (trace mode %d)" % t.traceMode()
    assert int(t.getRayTraceInfo().numRays) == n * SURFACE_RAYS_PER_POINT, who
    assert abs(t.getSourceArea() - SURFACE_AREA) <= 1e-5 * SURFACE_AREA, who
    assert (flux[mesh.part == cf.TOP] == 0).all(), who        # nothing inside the trench sees the top surface

    # the distinct emitters of the profile, ny of each
    key = np.stack([mesh.part[emit], np.round(pos, 6)], axis=1)
    uniq, first, count = np.unique(key, axis=0, return_index=True, return_counts=True)
    assert (count == cf.NY).all() and len(uniq) == 2 * (cf.W + 2 * cf.DEPTH)
    q_part, q_pos, q_W = mesh.part[emit][first], pos[first], W[first]
    arriving, V, _ = R.from_emitters(q_part, q_pos, q_W * 0.5)
    emitting_area = 0.5 * n
    C = SURFACE_AREA / emitting_area
    ratios, bounds, lines = [], [], []
    for row in S.rows:
        if row.key == "top":
            continue
        segs = (R.part == row.part) & (R.lo >= row.coord - 0.5 - 1e-9) & (R.hi <= row.coord + 0.5 + 1e-9)
        assert segs.sum() == R.m
        kw = float(arriving[segs].mean())
        v = V[segs].sum(axis=0)                                  # emitter -> the whole cell
        rays = cf.NY * SURFACE_RAYS_PER_POINT
        E = (rays * q_W * v).sum() ** 2 / (rays * q_W ** 2 * v).sum()
        bound = 5.0 / np.sqrt(E) + cf.REFERENCE_ERROR
        got = float(flux[row.idx].mean())
        ratios.append(got / kw)
        bounds.append(bound)
        lines.append("%s surface source: %-18s got %.5f  C K.W %.5f  ratio / C %+.4f  bound %.4f (%.0f %% of it)" % (
            who, row.label, got, C * kw, got / kw / C - 1, bound, 100 * abs(got / kw / C - 1) / bound))
    ratios, bounds = np.array(ratios), np.array(bounds)
    print("\n" + "\n".join(lines))
    print("%s surface source: C = %.5f, ratios %.5f .. %.5f, worst row uses %.0f %% of its bound" % (
        who, C, ratios.min(), ratios.max(), 100 * (np.abs(ratios / C - 1) / bounds).max()))
    bad = [ln for ln, r, b in zip(lines, ratios, bounds) if not abs(r / C - 1) <= b]
    assert not bad, "\n".join(bad)
    hi, lo = int(np.argmax(ratios)), int(np.argmin(ratios))
    assert (ratios[hi] - ratios[lo]) / C <= bounds[hi] + bounds[lo], (who, lines[hi], lines[lo])
