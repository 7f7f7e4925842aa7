"""CPU: the checker of the uv-space texel rasteriser checks what it claims to (texel_raster_cases.py).  A straightforward numpy float32 implementation of the
arithmetic include/texir_hip.h states for texir_texel_gbuffer passes the float64 oracle on every texel and equals the integer restatement of the crack and
overlap rules bit for bit on the exact cases; seven mutants of it -- centre at c / W, rows not flipped, highest id wins, >= on every edge, > on every edge,
barycentrics of unrotated corners, renormalised shading normals -- are rejected.  The caps on weak texels are asserted from the oracle alone.
No device is involved; test_gpu_texel_raster.py runs the same checks on the kernels."""
import re

import numpy as np
import pytest

import texel_raster_cases as C
from conftest import ROOT


def test_margin_comes_from_the_header():
    """the header states the bound the module's M rests on"""
    import os
    txt = open(os.path.join(ROOT, "include", "texir_hip.h")).read()
    assert re.search(r"m = \(8 D \+ 2\) 2\^-24", txt)
    assert "E = (x1 - x0) * (v - y0) - (y1 - y0) * (u - x0)" in txt
    assert (8 * 2.0 + 2) * C.U <= C.M <= 2.0 ** -18


@pytest.fixture(scope="module")
def room():
    mesh, sc = C.synth_mesh("room", 2000)
    return mesh, sc, C.Oracle(mesh, 128, 128)


def test_weak_cap_room(room):
    mesh, _, orc = room
    C.margin_of(mesh)
    assert orc.any_possible.sum() > 0.3 * 128 * 128
    print("room 2k 128^2 weak share %.4f" % orc.weak_share())
    assert orc.weak_share() <= C.CAP_WEAK


@pytest.mark.parametrize("normal", ["geometric", "shading"])
def test_restatement_passes_oracle_room(room, normal):
    mesh, _, orc = room
    out = C.raster_f32(mesh, 128, 128, normal)
    fails, worst = C.check_output(mesh, 128, 128, out, orc, normal)
    print(normal, worst)
    assert not fails, fails
    assert (out["prim"] >= 0).sum() > 0.3 * 128 * 128


def test_restatement_passes_oracle_odd_sizes():
    for mesh, H, W in C.odd_size_cases():
        C.margin_of(mesh)
        orc = C.Oracle(mesh, H, W)
        if H * W > 64:
            assert orc.weak_share() <= C.CAP_WEAK, (mesh.name, H, W, orc.weak_share())
        fails, _ = C.check_output(mesh, H, W, C.raster_f32(mesh, H, W), orc)
        assert not fails, (mesh.name, H, W, fails)


def test_restatement_equals_integer_rules_on_exact_cases():
    for mesh, H, W, k in C.exact_cases():
        own, count = C.raster_exact_int(mesh, H, W, k)
        out = C.raster_f32(mesh, H, W)
        assert np.array_equal(out["prim"], own), mesh.name
        if "overlapping" not in mesh.name:
            assert count.max() <= 1, mesh.name                     # every covered texel has exactly one owner


def test_exact_cases_cover_what_they_are_meant_to():
    cases = {m.name: (m, H, W, k) for m, H, W, k in C.exact_cases()}
    # interior of a grid: no texel lost, none given twice -- including centres on shared edges and on vertices
    for name in ("grid8_shared_edges", "grid16_on_centres", "grid16_fan", "grid8_mirrored"):
        m, H, W, k = cases[name]
        own, count = C.raster_exact_int(m, H, W, k)
        uv = m.tri_uvs
        cu, cv = (np.arange(W) + 0.5) / W, ((H - 1 - np.arange(H)) + 0.5) / H
        inner = ((cv > uv[:, 1].min()) & (cv < uv[:, 1].max()))[:, None] & ((cu > uv[:, 0].min()) & (cu < uv[:, 0].max()))[None, :]
        assert inner.sum() > 0 and (count[inner] == 1).all(), name
    # centres exactly on an edge / a vertex do occur
    m, H, W, k = cases["grid16_on_centres"]
    on_vertex = sum(1 for q in np.unique(m.tri_uvs, axis=0) if (q[0] * W - 0.5) % 1 == 0 and (q[1] * H - 0.5) % 1 == 0)
    assert on_vertex >= 15 * 15
    m, H, W, k = cases["one_triangle_whole_atlas"]
    assert (C.raster_exact_int(m, H, W, k)[0] == 0).all()
    m, H, W, k = cases["smaller_than_a_texel"]
    own, _ = C.raster_exact_int(m, H, W, k)
    assert 0 < (own >= 0).sum() < m.T                               # most triangles cover no centre at all
    m, H, W, k = cases["zero_area_and_nan"]
    own, _ = C.raster_exact_int(m, H, W, k)
    assert set(np.unique(own)) == {-1, 4}
    m, H, W, k = cases["two_charts_overlapping"]
    assert C.raster_exact_int(m, H, W, k)[1].max() >= 2


def _rejected_by_oracle(mesh, H, W, mutant, normal="geometric", rot=None):
    orc = C.Oracle(mesh, H, W)
    good, _ = C.check_output(mesh, H, W, C.raster_f32(mesh, H, W, normal, rot=rot), orc, normal)
    assert not good, good
    fails, _ = C.check_output(mesh, H, W, C.raster_f32(mesh, H, W, normal, mutant=mutant, rot=rot), orc, normal)
    return fails


def test_mutants_are_rejected(room):
    mesh, _, _ = room
    cases = {m.name: (m, H, W, k) for m, H, W, k in C.exact_cases()}
    assert _rejected_by_oracle(mesh, 128, 128, "centre_at_c_over_W")
    assert _rejected_by_oracle(mesh, 128, 128, "rows_not_flipped")
    m, H, W, _ = cases["two_charts_overlapping"]
    assert _rejected_by_oracle(m, H, W, "highest_id_wins")
    rot = np.arange(mesh.T) % 3
    assert _rejected_by_oracle(mesh, 128, 128, "bary_unrotated", rot=rot)
    assert _rejected_by_oracle(mesh, 128, 128, "renormalised_shading", normal="shading")
    # the two crack-rule mutants live inside the oracle's margin: the exact cases catch them bit for bit
    for mutant in ("ge_on_every_edge", "gt_on_every_edge"):
        caught = 0
        for m, H, W, k in C.exact_cases():
            own, _ = C.raster_exact_int(m, H, W, k)
            caught += not np.array_equal(C.raster_f32(m, H, W, mutant=mutant)["prim"], own)
        assert caught >= 3, mutant


def test_chart_border_cap(room):
    mesh, sc, orc = room
    near = C.chart_border_texels(sc, 128, 128)
    assert near.sum() / max(1, orc.any_possible.sum()) <= C.CAP_WEAK
