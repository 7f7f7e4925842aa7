"""No GPU: the reference of the occlusion query (tests/occlusion_cases.py) is sharp, its float32 restatement passes it, every mutant is rejected, it agrees
with light_cases.Ref's own visibility counts, the three new C-ABI names are declared and exported, and the `query` arguments are validated before any device
is touched.

Counted here from the reference alone (384 / 256 / 126 .. 600 rays per case, 15 cases, 2 to 6 segments each): no segment of any case has an uncertain ray
share above 2 %; the largest is 0.0 % on the sampled cases -- the segments' ends are placed beside the quantile rays' hits, not on them -- after the grid
cube's vertex / edge / face cases took the segments occlusion_cases.py gives them.
"""
import numpy as np
import pytest

import occlusion_cases as OC
import trace_cases as TC


@pytest.mark.parametrize("name", OC.NAMES)
def test_caps_and_agreement_with_the_cut_lists(name):
    c = OC.case(name)
    for tag, tn, tf in c.segments():
        occ, vis = c.classify(tn, tf)
        assert not (occ & vis).any()
        share = float((~occ & ~vis).mean())
        print("occlusion %-20s %-12s (%.6g, %.6g): occluded %.3f visible %.3f uncertain %.4f" % (name, tag, tn, tf, occ.mean(), vis.mean(), share))
        assert share <= OC.CAP_UNCERTAIN, (name, tag, share)
    # at t_near = 0 trace_cases' own lists, cut behind the closest robust hit, give the same classes
    rr = TC.RayRef(c.geo, c.org.astype(np.float64), c.dir.astype(np.float64))
    assert not rr.overflow.any()
    for tag, tn, tf in c.equal_segments():
        a, b = c.classify(0.0, tf), OC.classify_rayref(rr, tf)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (name, tag)


def closest_of(leaf):
    """the closest-hit answer of the restated leaf test: (t [R] f32 (inf: miss), pid [R])"""
    inside, t = leaf
    with np.errstate(invalid="ignore"):
        tt = np.where(inside & (t > 0), t, np.float32(np.inf)).astype(np.float32)
    j = tt.argmin(1)
    th = tt[np.arange(len(j)), j]
    return th, np.where(np.isfinite(th), j, -1)


@pytest.mark.parametrize("name", ["box_random", "patho_soup", "grid_vertices_edges", "grid_on_face", "grid_zero_nonfinite", "tie"])
def test_the_restated_leaf_test_is_trace_f32s(name):
    c = OC.case(name)
    t, pid = closest_of(c.leaf())
    t0, p0, _ = TC.trace_f32(c.geo, c.org, c.dir)
    assert np.array_equal(t.view(np.uint32), t0.view(np.uint32)) and np.array_equal(pid, p0)
    if name == "tie":
        assert (t[:4] == 0.5).all() and (t[6:10] == 0.25).all() and (pid[[4, 5, 10, 11]] == -1).all()


@pytest.mark.parametrize("name", OC.NAMES + ("tie",))
def test_occluded_f32_passes(name):
    c = OC.case(name)
    leaf = c.leaf()
    if name != "tie":
        for tag, tn, tf in c.segments():
            OC.check_certain(*c.classify(tn, tf), OC.occluded_f32(c.geo, c.org, c.dir, tn, tf, leaf=leaf), "%s %s" % (name, tag))
    t, pid = closest_of(leaf)
    for tag, tn, tf in (c.equal_segments() if name != "tie" else [("tie", 0.0, OC.TIE_FAR)]):
        OC.equals_closest(OC.occluded_f32(c.geo, c.org, c.dir, 0.0, tf, leaf=leaf), t, pid, tf, "%s %s" % (name, tag))
    # a segment that holds nothing
    assert not OC.occluded_f32(c.geo, c.org, c.dir, 0.5, 0.5, leaf=leaf).any() and not OC.occluded_f32(c.geo, c.org, c.dir, 0.0, float("nan"), leaf=leaf).any()


@pytest.mark.parametrize("mut,name,tag,by", OC.MUTANT_CASES, ids=[m[0] for m in OC.MUTANT_CASES])
def test_every_mutant_is_rejected(mut, name, tag, by):
    c = OC.case(name)
    leaf = c.leaf()
    if by == "closest":
        tn, tf = 0.0, OC.TIE_FAR
        t, pid = closest_of(leaf)
        ok = lambda got: OC.equals_closest(got, t, pid, tf, name)
    else:
        tn, tf = {s[0]: s[1:] for s in c.segments()}[tag]
        ok = lambda got: OC.check_certain(*c.classify(tn, tf), got, name)
    ok(OC.occluded_f32(c.geo, c.org, c.dir, tn, tf, leaf=leaf))
    assert TC.rejected(ok, OC.occluded_f32(c.geo, c.org, c.dir, tn, tf, mut=mut, leaf=leaf)), mut


@pytest.mark.parametrize("name,traced,visible", [("room_quad", 29167, 14974), ("room_sphere", 18246, 9531)])
def test_agrees_with_the_light_references_own_counts(name, traced, visible):
    import light_cases as LC
    c, rr, mask = OC.light_rays(name)
    ref = c.ref()
    occ, vis = OC.classify_rayref(rr, c.t_max)
    assert rr.R == traced == int(ref.traced_maybe.sum()) and np.array_equal(mask, ref.traced_maybe[0])
    # the light reference's classes are this module's: certainly occluded, possibly occluded
    assert np.array_equal(occ, (ref.traced_maybe & ~ref.vis_maybe)[0][mask]) and np.array_equal(~occ & ~vis, ref.uncertain_vis[0][mask])
    assert int((~occ).sum()) == visible == int(ref.vis_maybe.sum())
    print("occlusion %s: %d rays, %d certainly occluded (%.1f %%), %d uncertain" % (name, traced, occ.sum(), 100.0 * occ.mean(), (~occ & ~vis).sum()))
    assert float((~occ & ~vis).mean()) <= LC.CAP_UNCERTAIN_SAMPLES


def test_the_three_entry_points_are_declared_and_exported():
    import test_cabi
    from texir_code_amd import _lib
    syms = test_cabi.declared_symbols()
    L = _lib.lib()
    for s in ("texir_trace_occluded", "texir_irt_lights_any", "texir_atlas_bake_any"):
        assert s in syms and hasattr(L, s), s
        assert getattr(L, s).argtypes is not None
    assert L.texir_irt_lights_any.argtypes == L.texir_irt_lights.argtypes and L.texir_atlas_bake_any.argtypes == L.texir_atlas_bake.argtypes
    test_cabi.test_header_symbols_exported()


def test_query_arguments_are_validated_without_a_device():
    from texir_code_amd import atlas, models, scene, tools
    assert scene.check_query("any") is True and scene.check_query("closest") is False
    for bad in ("Any", "", None, "first", 1):
        with pytest.raises(ValueError, match="'closest' or 'any'"):
            scene.check_query(bad)
    with pytest.raises(ValueError, match="'closest' or 'any'"):
        scene.Scene.irt_lights(object(), None, None, None, None, 16, query="nearest")
    with pytest.raises(ValueError, match="'closest' or 'any'"):
        atlas.bake_atlas(object(), None, None, None, None, None, query="nearest")
    assert models.irt_light_query("closest") == "closest" and models.irt_light_query(" ANY ") == "any"
    with pytest.raises(ValueError, match="train.irt_light_query"):
        models.irt_light_query("both")
    assert tools.parse_bake_atlas(["root", "64"])["query"] == "closest"
    assert tools.parse_bake_atlas(["root", "64", "--query", "any"])["query"] == "any" and tools.parse_bake_atlas(["root", "64x32", "--query=any"])["query"] == "any"
    with pytest.raises(ValueError, match="--query"):
        tools.parse_bake_atlas(["root", "64", "--query", "all"])
    assert tools.main(["bake-atlas", "root", "64", "--query", "all"]) == 2
