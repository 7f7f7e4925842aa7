"""The checker of the cube G-buffer proved WITHOUT a GPU (tests/gbuffer_cases.py holds the reference, the bounds and the rules).

  * the exact rational inverse is an inverse; the rays it gives are pinned against the independent two-depth unprojection of oracle/ref_torch.gbuffer
    (its nested `rays`, restated here in float64: near and far point of the pixel through numpy's inverse): directions parallel and of the same sense,
    origins on the same line;
  * the analytic uv_da is pinned against central differences of the float64 uv on the hit triangle's plane at steps h and h / 2: the disagreement
    shrinks by about four per halving, so the pin has no tolerance of its own.  Accepted shrink: 3 to 5, for every entry whose disagreement at h is
    above the floor 1e-10 (1 + the pixel's largest |uv_da|), below which float64 noise of the differences (2^-53 |uv| / h) decides the ratio; an entry
    below the floor at h must stay below it at h / 2 (uv is exactly linear where the triangle is parallel to the image plane);
  * the caps of gbuffer_cases hold for every case of the GPU module, D_min >= 0.05 included;
  * the library's double stage restated (invert4, basis_double) stays inside half the stated allowance E64;
  * gbuffer_f32, the float32 restatement of the header's algorithm, passes every case in both normal modes and both flip_v values;
  * every mutant of gbuffer_f32 is rejected on at least one case;
  * the two mvps the library must refuse are refused by the restated host code.

Measured (the reference alone, 22 cases): no ray overflows; pixels with more than one outcome at most 1.85 % of a case that is not aimed (box_graze_c3: one pixel
of 54; every other one at most 0.78 %), 17 % to 100 % of the six aimed ones (box_centre_c17 .. c1); sharp pixels 100 % of a case's hits but for the scan (99.8 %,
99.9 %); D_min 0.06 (the grazing eye), 0.073 and 0.145 (room), 0.46 (scan), 0.69 (the far eye), 1 (the centre).  The central differences shrink by 3.998 to 4.009.
gbuffer_f32's worst error / bound: position 0.049, uv 0.061, uv_da 0.036, interpolated normal 0.019, geometric normal 0.056.  The module takes 6 s.
"""
import fractions

import numpy as np
import pytest

import gbuffer_cases as GC
import trace_cases as TC


def test_case_names_are_complete():
    assert sorted(GC.cases()) == sorted(GC.NAMES)


def test_exact_inverse_is_an_inverse():
    Fr = fractions.Fraction
    for name in ("box_graze_rot_c17", "box_far_c8", "scan_rot_proj_c16"):
        for m in GC.cases()[name].mvp:
            inv = GC.inverse_exact(m)
            M = [[Fr(float(x)) for x in row] for row in m]
            for r in range(4):
                for c in range(4):
                    assert sum(inv[r][k] * M[k][c] for k in range(4)) == (1 if r == c else 0)
    for name, mvp in GC.bad_mvps().items():
        assert any(GC.basis_exact(m) is None for m in mvp), name


def test_point_mesh_distance():
    V = np.array([[[0, 0, 0], [2, 0, 0], [0, 2, 0]]], np.float64)
    assert GC.point_mesh_distance((0.5, 0.5, 3.0), V) == 3.0                       # above the interior: the plane
    assert abs(GC.point_mesh_distance((1.0, -4.0, 3.0), V) - 5.0) < 1e-15          # beyond an edge: the edge, not a vertex (sqrt(26), sqrt(26) from the two)
    assert abs(GC.point_mesh_distance((-3.0, -4.0, 0.0), V) - 5.0) < 1e-15         # beyond a corner
    assert abs(GC.point_mesh_distance((2.0, 2.0, 0.0), V) - np.sqrt(2.0)) < 1e-15  # beyond the hypotenuse, in the plane


@pytest.mark.parametrize("name", GC.NAMES)
def test_rays_against_two_depth_unprojection(name):
    case = GC.cases()[name]
    ref = case.ref()
    minv = np.linalg.inv(case.mvp.astype(np.float64))
    one = np.ones_like(ref.x)
    a = np.einsum("rk,rkl->rl", np.stack([ref.x, ref.y, -one, one], 1), minv[ref.face])
    b = np.einsum("rk,rkl->rl", np.stack([ref.x, ref.y, one, one], 1), minv[ref.face])
    O, far = a[:, :3] / a[:, 3:], b[:, :3] / b[:, 3:]
    D = far - O
    unit = lambda v: v / np.linalg.norm(v, axis=1, keepdims=True)
    scale = max(1.0, float(np.abs(ref.eye).max()))
    assert np.linalg.norm(np.cross(unit(D), unit(ref.d)), axis=1).max() < 1e-9 * scale
    assert ((D * ref.d).sum(1) > 0).all()
    # the near point lies on the reference's line: its offset from the eye (about the near distance long) has no component across the direction
    off = O - ref.eye
    assert np.linalg.norm(np.cross(off, unit(ref.d)), axis=1).max() < 1e-9 * scale
    assert ((off * ref.d).sum(1) > 0).all()


@pytest.mark.parametrize("name", [n for n in GC.NAMES if n != "box_stride_c296"])
def test_uv_da_against_central_differences(name):
    case = GC.cases()[name]
    ref, geo, c = case.ref(), case.geo, case.c
    ry = ref.rays
    rows = np.nonzero(ry.n > 0)[0]
    k0 = np.zeros(rows.size, np.int64)
    da, _ = ref.outputs(rows, k0, None, False)["uv_da"]
    pid = ry.id[rows, 0].astype(np.int64)
    P = geo.verts.astype(np.float64)[geo.tris[pid]]
    T = geo.tri_uvs.astype(np.float64).reshape(-1, 3, 2)[pid]
    g = lambda name_: np.stack([getattr(b, name_) for b in ref.exact])[ref.face[rows]]
    d0, dx, dy, eye = g("d0"), g("dx"), g("dy"), g("eye")

    def uv_at(x, y):
        d = d0 + x[:, None] * dx + y[:, None] * dy
        e1, e2, tv = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0], eye - P[:, 0]
        pv = np.cross(d, e2)
        det = (e1 * pv).sum(1)
        u = (tv * pv).sum(1) / det
        v = (d * np.cross(tv, e1)).sum(1) / det
        return T[:, 0] * (1 - u - v)[:, None] + T[:, 1] * u[:, None] + T[:, 2] * v[:, None]

    def cd(h):
        s = h * 2.0 / c                                                            # h pixels in ndc
        x, y = ref.x[rows], ref.y[rows]
        gx = (uv_at(x + s, y) - uv_at(x - s, y)) / (2 * h)
        gy = (uv_at(x, y + s) - uv_at(x, y - s)) / (2 * h)
        return np.stack([gx[:, 0], gy[:, 0], gx[:, 1], gy[:, 1]], 1)
    h = 2.0 ** -6
    e1, e2 = np.abs(cd(h) - da), np.abs(cd(h / 2) - da)
    floor = 1e-10 * (1 + np.abs(da).max(1, keepdims=True)) * np.ones_like(da)
    above = e1 > floor
    assert (e2[~above] <= floor[~above]).all()
    ratio = e1[above] / e2[above]
    print("uv_da pin %-20s %d of %d entries above the floor, shrink %.3f .. %.3f" % (name, above.sum(), above.size, ratio.min() if ratio.size else 4, ratio.max() if ratio.size else 4))
    assert ((ratio >= 3) & (ratio <= 5)).all()
    if any(k in name for k in ("rot", "scaled", "proj")):                          # (without a rotation most walls are parallel to an image plane: uv is linear there)
        assert above.mean() > 0.5


@pytest.mark.parametrize("name", GC.NAMES)
def test_caps(name):
    case = GC.cases()[name]
    overflow, multi, sharp, d_min = case.ref().caps()
    print("caps %-20s overflow %d, more than one outcome %.4f, sharp %.4f, D_min %.4f" % (name, overflow, multi, sharp, d_min))
    assert overflow == 0
    assert case.aimed or multi <= GC.CAP_MULTI
    assert sharp >= GC.CAP_SHARP
    assert d_min >= GC.D_MIN
    if case.closed:
        assert (case.ref().rays.n > 0).all()                                       # a closed mesh from inside: every pixel has a candidate


@pytest.mark.parametrize("name", GC.NAMES)
def test_double_stage_inside_half_its_allowance(name):
    case = GC.cases()[name]
    for f in range(6):
        ex = case.ref().exact[f]
        eye, dx, dy, d0, sgn = GC.basis_double(case.mvp[f])
        assert sgn == ex.sgn
        L = np.linalg.norm(d0)
        e64 = GC.e64_of(case.mvp[f])
        for got, want in ((dx, ex.dx), (dy, ex.dy), (d0, ex.d0)):
            assert np.abs(np.array(got) / L - want).max() <= 0.5 * e64
        assert np.abs(np.array(eye) - ex.eye).max() <= 0.5 * e64 * max(1.0, np.abs(ex.eye).max())
        assert e64 < 2.0 ** -26                                                    # the allowance stays below a quarter of float32's unit roundoff


def test_sgn_is_negative_somewhere():
    assert sorted({GC.cases()["box_scaled_c8"].ref().exact[f].sgn for f in range(6)}) == [-1, 1]


@pytest.mark.parametrize("flip_v", [0, 1])
@pytest.mark.parametrize("normals", ["geometric", "interpolated"])
@pytest.mark.parametrize("name", GC.NAMES)
def test_gbuffer_f32_inside_every_bound(name, normals, flip_v):
    case = GC.cases()[name]
    cn = GC.corner_normals(case.geo) if normals == "interpolated" else None
    worst = GC.check_gbuffer(case, GC.gbuffer_f32(case, cn, flip_v), cn, flip_v, "gbuf_f32")
    assert all(w < 1 for w in worst.values())


MUTANT_CASES = ("box_graze_c8", "box_scaled_c8", "scan_c16")


@pytest.mark.parametrize("mut", GC.MUTANTS)
def test_mutants_are_rejected(mut):
    hits = []
    for name in MUTANT_CASES:
        case = GC.cases()[name]
        for cn in (None, GC.corner_normals(case.geo)):
            if TC.rejected(GC.check_gbuffer, case, GC.gbuffer_f32(case, cn, 1, mut), cn, 1, "gbuf_mut", mut):
                hits.append((name, cn is not None))
    print("mutant %-18s rejected on %s" % (mut, hits))
    assert hits


def test_refused_mvps_are_refused_by_the_restated_host_code():
    bad = GC.bad_mvps()
    assert [GC.invert4(m) is None for m in bad["singular"]] == [False, False, False, True, False, False]
    for m in bad["affine"]:
        inv = GC.invert4(m)
        assert inv is not None and inv[2][3] == 0.0 and GC.basis_double(m) is None
