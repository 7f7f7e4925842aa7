"""gbuffer_kernel<4> / <2> and launch_gbuffer's host inversion (csrc/gbuffer.hip; gbuffer.cast_gbuffer) against the float64 reference of tests/gbuffer_cases.py:
EVERY pixel by the per-pixel rule (the triangle by check_hits' rule, position, normal, uv and uv_da inside bounds derived from the reference alone, background
exact, no leak out of a closed mesh).  The bounds and caps are derived in gbuffer_cases.py and proved on the CPU by test_gbuffer_ref_cpu.py.

Cases: the closed 192-triangle cube from its centre (axis rays through shared vertices) and from 0.06 off a wall at c = 1, 2, 3, 5, 8, 17; seeded general
rotations; an eye 1000 units from the origin; mvp scaled by +-3; a projection with n = 1e-2, f = 10; the golden room from two eyes and a 6000-triangle scan
with openings at c = 16; c = 296 for the grid-stride loop's second trip.  Every case runs with flip_v 0 and 1, on a fresh scene (geometric normals) and
after set_corner_normals (interpolated, not renormalised).

MEASURED on an MI355X (36 tests, all passing, 4 s; worst error / bound per output, 1.0 = the bound; every pixel compared, none rejected):
    output                  22 cases x 2 normal modes x 2 flip_v       four tree builds (cube c = 8, room c = 16)
    position                0.049  (room_a_c16)                        0.049
    uv                      0.061  (room_a_c16, flip_v = 1)            0.061
    uv_da                   0.039  (box_scaled_c8)                     0.026
    normal, interpolated    0.020  (room_b_rot_c16)                    0.014
    normal, geometric       0.054  (scan_rot_proj_c16)                 0.047
    triangle                every tri_id a candidate no robust hit shadows; no background pixel inside the closed cube, the rays through shared vertices included
The geometric normal has the caller's winding on every slot, odd slots and rotated records included; a singular or affine mvp returned TEXIR_ERR_HIP before
this module and returns TEXIR_ERR_INVALID now (texir_gbuffer_cast checks the mvp before it launches).
"""
import numpy as np
import pytest
import torch

import gbuffer_cases as GC
import trace_cases as TC

pytestmark = pytest.mark.gpu

KEYS = ("position", "normal", "mask", "uv", "uv_da", "tri_id")


def gpu_scene(tx, geo):
    return tx.Scene(geo.verts, geo.tris, geo.tri_uvs, geo.hdr)


def cast(sc, case, flip_v):
    from texir_code_amd import gbuffer as GB
    out = GB.cast_gbuffer(sc, torch.from_numpy(case.mvp), case.c, flip_v=bool(flip_v))
    c = case.c
    assert out["position"].shape == (6, c, c, 3) and out["uv_da"].shape == (6, c, c, 4) and out["tri_id"].shape == (6, c, c) and out["tri_id"].dtype == torch.int32
    return {k: out[k].cpu().numpy() for k in KEYS}


def check_both_normal_modes(tx, case, family, what="", flips=(0, 1)):
    """a fresh scene has no corner normals: the geometric branch; then the same scene with corner normals set"""
    from texir_code_amd import gbuffer as GB
    sc = gpu_scene(tx, case.geo)
    for flip_v in flips:
        GC.check_gbuffer(case, cast(sc, case, flip_v), None, flip_v, family, what)
    cn = GC.corner_normals(case.geo)
    GB.set_corner_normals(sc, cn)
    for flip_v in flips:
        GC.check_gbuffer(case, cast(sc, case, flip_v), cn, flip_v, family, what)
    return sc


@pytest.mark.parametrize("name", GC.NAMES)
def test_gbuffer_per_pixel(tx, name):
    case = GC.cases()[name]
    if name == "box_stride_c296":
        P = 6 * case.c * case.c
        assert P > GC.STRIDE_START and (case.pix >= GC.STRIDE_START).sum() == P - GC.STRIDE_START     # every pixel of the second trip is compared
    check_both_normal_modes(tx, case, "gbuf")


def test_corner_normals_set_twice_the_second_set_wins(tx):
    from texir_code_amd import gbuffer as GB
    case = GC.cases()["box_graze_c8"]
    sc = gpu_scene(tx, case.geo)
    first, second = GC.corner_normals(case.geo, seed=12), GC.corner_normals(case.geo)
    GB.set_corner_normals(sc, first)
    out = cast(sc, case, 1)
    GC.check_gbuffer(case, out, first, 1, "gbuf", "first set")
    GB.set_corner_normals(sc, second)
    out = cast(sc, case, 1)
    GC.check_gbuffer(case, out, second, 1, "gbuf", "second set")
    assert TC.rejected(GC.check_gbuffer, case, out, first, 1, "gbuf_mut", "second set against the first normals")


BUILDS = [("TEXIR_BVH_WIDTH", "2"), ("TEXIR_UNIFORM_FLOAT", "0"), ("TEXIR_MAX_LEAF", "1"), ("TEXIR_MAX_LEAF", "8")]


@pytest.mark.parametrize("var,value", BUILDS)
@pytest.mark.parametrize("name", ["box_graze_c8", "room_a_c16"])
def test_gbuffer_per_pixel_other_tree_builds(tx, monkeypatch, name, var, value):
    """gbuffer_kernel<2> on the binary tree, no float node copy, leaves of one and of up to eight triangles: the switch is set before the scene is made"""
    monkeypatch.setenv(var, value)
    check_both_normal_modes(tx, GC.cases()[name], "gbuf_build", "%s=%s" % (var, value))


def test_two_calls_and_another_stream_give_the_same_bits(tx):
    case = GC.cases()["room_b_rot_c16"]
    sc = gpu_scene(tx, case.geo)
    a, b = cast(sc, case, 1), cast(sc, case, 1)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        c = cast(sc, case, 1)
    st.synchronize()
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes() and a[k].tobytes() == c[k].tobytes(), k
    GC.check_gbuffer(case, c, None, 1, "gbuf", "non-default stream")


@pytest.mark.parametrize("which", ["singular", "affine", "c=0", "c=16385"])
def test_refused_arguments_return_invalid_and_write_nothing(tx, which):
    from texir_code_amd import _lib
    case = GC.cases()["box_graze_c8"]
    sc = gpu_scene(tx, case.geo)
    c = {"c=0": 0, "c=16385": 16385}.get(which, case.c)
    mvp = np.ascontiguousarray(GC.bad_mvps().get(which, case.mvp), np.float32)
    P = 6 * case.c * case.c
    fill = 7.25
    bufs = [torch.full((P, k), fill, device="cuda") for k in (3, 3, 1, 2, 4)]
    tri = torch.full((P,), 77, device="cuda", dtype=torch.int32)
    rc = _lib.lib().texir_gbuffer_cast(sc.h, _lib.ptr(mvp), c, 1, *[_lib.ptr(b) for b in bufs], _lib.ptr(tri), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1, rc                                                            # TEXIR_ERR_INVALID (include/texir_hip.h)
    assert all(bool((b == fill).all()) for b in bufs) and bool((tri == 77).all())
    # the scene is still good for a valid call
    GC.check_gbuffer(case, cast(sc, case, 0), None, 0, "gbuf", "after a refused call (%s)" % which)
