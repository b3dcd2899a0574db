"""The CPU oracle against the closed forms of tests/closed_forms.py.

Every device result of the suite is pinned to the oracle; this file holds the oracle itself to physics that was not
derived from it: the 2-D radiosity system for diffuse particles (the diffuse reflection law, the (1 - sticking) weight
chain, reflective and periodic continuation, normalizeFlux(SOURCE)), mirror images for specular particles (the specular
law, the same chain) and the in-plane angle integral for a cos^n source (the source's angular law).  The device is held
to the same references, through the same builders and tolerances, in tests/test_closed_form_flux.py.

    python -m pytest tests/test_closed_form_flux_host.py -q -s      prints every row and the share of its bound used
    python tests/test_closed_form_flux_host.py scatter              re-measures closed_forms.SCATTER (8 seeds, CPU)
"""
import os
import sys

import numpy as np
import pytest

import closed_forms as cf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import pyoracle as po   # noqa: E402


def run_oracle(case_id, num_rays=cf.HOST_RAYS, seed=cf.SEED):
    case = cf.CASES[cf.CASE_IDS.index(case_id)]
    S = cf.scene_of(case_id)
    o = po.Oracle()
    if S.kind == "mesh":
        o.set_triangles(S.geom.verts, S.geom.tris, 1.0, 3)
    else:
        o.set_disks(S.geom.points, S.geom.normals, 1.0, S.D)
    o.set_boundary_conditions(S.bcs)
    if S.source_direction is not None:
        o.set_source_direction(S.source_direction)
    o.set_particle(po.DIFFUSE if case.particle == cf.DIFFUSE else po.SPECULAR, case.sticking, case.power)
    o.set_num_rays_fixed(num_rays)
    o.set_rng_seed(seed)
    o.set_lazy_rng(True)
    o.apply(po.max_threads())
    if S.kind == "disks":
        assert abs(o.disk_radius() - S.geom.radius) <= 1e-6 * S.geom.radius
    assert abs(o.source_area() - S.source_area) <= 1e-5 * S.source_area
    return o.normalize_flux(o.flux())


def test_the_scenes_are_what_the_references_assume():
    m = cf.trench_mesh()
    assert len(m.tris) == 640
    c, n = cf.triangle_centroids(m)
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0)                # unit quads: two triangles of area 1/2
    want = {cf.TOP: (0, 0, 1), cf.BOTTOM: (0, 0, 1), cf.LEFT: (1, 0, 0), cf.RIGHT: (-1, 0, 0)}
    for p, nn in want.items():                                       # wound towards the open side
        assert (n[m.part == p] == np.asarray(nn, dtype=np.float64)).all(), p
    assert (c[m.part == cf.BOTTOM][:, 2] == -cf.DEPTH).all() and (np.abs(c[m.part == cf.LEFT][:, 0]) == cf.W / 2).all()
    for D in (3, 2):
        g = cf.trench_disks(D)
        up = 2 if D == 3 else 1
        top, wall = g.part == cf.TOP, (g.part == cf.LEFT) | (g.part == cf.RIGHT)
        assert np.abs(g.points[top][:, 0]).min() - g.radius >= cf.W / 2 - 1e-6     # no disc overhangs the opening
        assert g.points[wall][:, up].max() + g.radius <= 1e-6
        assert g.points[wall][:, up].min() - g.radius < -cf.DEPTH                  # the walls are covered to the bottom
        assert len(cf.disk_excluded(g)) == 4 and len({c for _, c in cf.disk_excluded(g)}) == 3   # 3 rows of the profile
        o = cf.trench_disks(D, overhang=True)
        assert abs(cf.W / 2 - (np.abs(o.points[o.part == cf.TOP][:, 0]).min() - o.radius) - (o.radius - 0.5)) < 1e-6


def test_the_references_agree_with_each_other_and_converge():
    """m = 40 against m = 80: every row mean within 1e-3 (half of closed_forms.REFERENCE_ERROR); and where two
    references describe the same thing they agree: at sticking 1 the radiosity bottom is the power-1 integral and the
    k = 0 image; energy is conserved (what the opening lets in is absorbed or leaves again)."""
    w, d = cf.W, cf.DEPTH
    for s in (1.0, 0.2):
        for scallop in (None, (cf.scallop_depth(cf.disk_radius(3)), cf.W / 2 + cf.disk_radius(3) + 4)):
            a, b = cf.radiosity(w, d, s, 40, scallop), cf.radiosity(w, d, s, 80, scallop)
            worst = 0.0
            for half in (0.5, cf.disk_radius(2), cf.disk_radius(3)):
                for part, lo, hi in ((cf.BOTTOM, -w / 2, w / 2), (cf.LEFT, -d, 0.0), (cf.RIGHT, -d, 0.0)):
                    for c in np.arange(lo + 0.5, hi, 1.0):
                        ra, rb = a.row_mean(part, c - half, c + half), b.row_mean(part, c - half, c + half)
                        worst = max(worst, abs(ra / rb - 1.0))
            print("radiosity s=%.1f scallop=%s: m=40 against m=80, worst row %.2e" % (s, scallop is not None, worst))
            assert worst < 1e-3
    R = cf.radiosity(w, d, 1.0)
    x = R.mid[R.part == cf.BOTTOM][:, 0]
    assert np.abs(R.F[R.part == cf.BOTTOM] - cf.power_cosine_bottom(w, d, 1.0, x)).max() < 1e-12
    assert np.abs(cf.specular_bottom(w, d, 1.0, x) - cf.power_cosine_bottom(w, d, 1.0, x)).max() < 1e-12
    for s in (1.0, 0.2):
        R = cf.radiosity(w, d, s)
        absorbed = s * R.F.sum() / R.m
        back_out = (1 - s) * (R.F * R.F_direct).sum() / R.m       # reciprocity: a segment's view of the opening
        print("radiosity s=%.1f: absorbed %.5f + leaving %.5f of %d entering" % (s, absorbed, back_out, w))
        assert abs(absorbed + back_out - w) < 2e-3 * w
    # the second Neumann term on the discretisation, and from point emitters on the segments' midpoints
    R = cf.radiosity(w, d, 1.0)
    direct, _, _ = R.direct_at(R.part, 0.5 * (R.lo + R.hi))
    assert np.abs(direct - R.F_direct).max() < 1e-12
    second, _, _ = R.from_emitters(R.part, 0.5 * (R.lo + R.hi), R.F_direct / R.m)
    from_corner = np.where(R.part == cf.BOTTOM, w / 2 - np.abs(R.mid[:, 0]), R.mid[:, 1] + d)
    assert np.abs(second / R.second_term() - 1.0)[from_corner > 0.5].max() < 2e-3   # (a point is no segment close by)


def test_the_recorded_offset_of_the_3d_disk_cloud_is_what_the_scallop_terms_add():
    for s, want in cf.DISK3_SCALLOP_OFFSET.items():
        S = cf.scene_of("disks3-diffuse-%.1f" % s)
        plain = cf.radiosity(cf.W, cf.DEPTH, s)
        r = S.geom.radius
        for key in ("bottom", "wall"):
            fold = [row.ref / plain.row_mean(row.part, row.coord - r, row.coord + r) - 1.0
                    for row in S.rows if row.key == key]
            print("disks3 s=%.1f %-6s scallop terms add %+.4f .. %+.4f, mean %+.4f" % (
                s, key, min(fold), max(fold), np.mean(fold)))
            assert abs(np.mean(fold) - want[key]) < 1e-4


@pytest.mark.parametrize("case_id", cf.CASE_IDS)
def test_oracle_matches_the_closed_form(case_id):
    flux = run_oracle(case_id)
    report, failures, worst = cf.compare(case_id, flux, cf.HOST_RAYS, "oracle")
    print("\n" + "\n".join(report))
    assert not failures, "\n".join(failures)


def measure_scatter():
    for case_id in cf.SCATTER:
        S = cf.scene_of(case_id)
        runs = np.array([[run_oracle(case_id, seed=seed)[row.idx].astype(np.float64).mean() for row in S.rows]
                         for seed in cf.SCATTER_SEEDS])
        rel = runs.std(axis=0, ddof=1) / runs.mean(axis=0)
        bias = runs.mean(axis=0) / np.array([row.ref for row in S.rows]) - 1.0
        out = {}
        for key in ("top", "bottom", "wall"):
            sel = [i for i, row in enumerate(S.rows) if row.key == key]
            if sel:
                out[key] = round(float(rel[sel].max()), 5)
                print("   %-6s mean over seeds against the reference: %+.4f .. %+.4f (mean %+.4f)" % (
                    key, bias[sel].min(), bias[sel].max(), bias[sel].mean()))
        print('    "%s": %s,' % (case_id, out))


if __name__ == "__main__":
    if sys.argv[1:] == ["scatter"]:
        measure_scatter()
    else:
        sys.exit(__doc__)
