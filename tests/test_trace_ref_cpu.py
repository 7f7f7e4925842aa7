"""The checker of the closest-hit and IrT kernels proved WITHOUT a GPU (tests/trace_cases.py holds the reference, the bounds and the rules).

  * oracle/texir_oracle.c txo_ray_candidates is pinned against the numpy restatement trace_cases.candidates_numpy;
  * a float32 brute-force transcription of the documented watertight algorithm (trace_f32), a float32 query_irf (shade_f32) and a float32 estimator
    (estimator_f32), written op by op in numpy, are accepted with no ray and no texel left out;
  * the C oracle's float32 BVH results (cast_rays / irt_generate, tracer="bvh": Moeller-Trumbore, not watertight) go through the same check with the
    same K.  Rejections: none -- every ray and every texel of every case here is accepted (the oracle's leaks through shared edges need rays aimed at
    them within float32 rounding; on the aimed cases below its closest hit is still a candidate);
  * every mutant is rejected in at least one ray or texel of every case it applies to.  Whether a shading mutant applies to a case is decided from the
    reference alone: it does where the mutated float64 radiance of a ray's closest robust hit leaves the reference's own bound;
  * the caps of trace_cases are computed and asserted for every sampled case, the GPU module's IrT cases included.  The cases AIMED at shared vertices,
    edges and faces have several candidates per ray by construction (that is what they are for): the share is printed, the cap is for sampled rays.

Measured (the reference alone, 8 CPU threads): no ray of any case overflows its list; rays with more than one outcome at most 1.6 % of a sampled ray case
here (the 3000 stacked triangles, 256 rays; 0.57 % at the GPU module's 3000 rays; every other sampled case at most 0.33 %; cap 2 %), samples with more than
one outcome at most 0.11 % of an IrT case; texels that are not sharp at most 4.3 % of a case (room, 70 texels x 512 samples; cap 20 %).  The references of
all the GPU module's cases take 75 s.
"""
import numpy as np
import pytest

import trace_cases as TC
from texture_cases import K, TINY, U

AIMED = ("grid_vertices_edges", "grid_axis_parallel", "grid_on_face")
_CASES = {}


def cases():
    if not _CASES:
        for c in TC.ray_cases(small=True):
            _CASES[c.name] = c
    return _CASES


NAMES = ["room_random", "room_hemisphere", "box_random", "box_hemisphere", "house_random", "scan_random", "patho_stack", "patho_fan", "patho_soup", "patho_single",
         "grid_vertices_edges", "grid_axis_parallel", "grid_on_face", "grid_unnormalised", "grid_zero_nonfinite"]
_F32 = {}


def traced(name):
    if name not in _F32:
        c = cases()[name]
        _F32[name] = TC.trace_f32(c.geo, c.org, c.dir)
    return _F32[name]


def test_case_names_are_complete():
    assert sorted(cases()) == sorted(NAMES)


@pytest.mark.parametrize("scene", ["room", "grid", "stack"])
def test_c_candidates_match_the_numpy_restatement(scene):
    rng = np.random.default_rng(1)
    if scene == "room":
        geo, gb = TC.golden_geo("room")
        v = np.argwhere(gb["valid"].reshape(-1) > 0)[:, 0]
        org, d = gb["pos"].reshape(-1, 3)[rng.choice(v, 300)].astype(np.float64), TC._random_dirs(rng, 300).astype(np.float64)
        bd = np.abs(d) * 1e-7 + 1e-9                          # a direction bound as the IrT rays carry one
    else:
        c = cases()["grid_vertices_edges" if scene == "grid" else "patho_stack"]
        geo, org, d, bd = c.geo, c.org[:150].astype(np.float64), c.dir[:150].astype(np.float64), None
    got = geo.osc().ray_candidates(org, d, K, U, TINY, bd, 64)
    ref = TC.candidates_numpy(geo, org, d, bd)
    assert not got["overflow"].any()
    assert np.array_equal(got["n"], ref["cand"].sum(1))
    assert np.array_equal(got["any_robust"], ref["robust"].any(1))
    assert got["n"].max() >= (2 if scene != "room" else 1)
    for r in range(len(org)):
        ids = np.nonzero(ref["cand"][r])[0]
        ids = ids[np.lexsort((ids, ref["t"][r, ids]))]
        n = len(ids)
        assert np.array_equal(got["id"][r, :n], ids) and (got["id"][r, n:] == -1).all(), r
        for f in ("t", "u", "v", "minb", "m", "bt"):
            assert np.allclose(got[f][r, :n], ref[f][r, ids], rtol=1e-9, atol=1e-300), (r, f)
        for k in range(3):
            assert np.allclose(got["b%d" % k][r, :n], ref["b"][r, ids, k], rtol=1e-9, atol=1e-300), (r, k)
        assert np.array_equal(got["robust"][r, :n] > 0, ref["robust"][r, ids]), r
        rob = np.nonzero(ref["robust"][r])[0]
        assert (got["t_rob"][r] == ref["t"][r, rob].min()) if len(rob) else np.isinf(got["t_rob"][r]), r


@pytest.mark.parametrize("name", NAMES)
def test_float32_transcription_and_oracle_bvh_are_accepted_and_caps_hold(name):
    c = cases()[name]
    ref = c.ref()
    over, multi = TC.ray_caps(ref)
    print("caps %-22s overflow %d, rays with more than one outcome %.4f" % (name, over, multi))
    assert over == 0
    if name not in AIMED:
        assert multi <= TC.CAP_MULTI
    t, pid, uv = traced(name)
    TC.check_hits(ref, t, pid, uv, TC.shade_f32(c.geo, t, pid, uv), "f32", name)
    osc = c.geo.osc()
    tb, pb, uvb = osc.cast_rays(c.org, c.dir, tracer="bvh")
    TC.check_hits(ref, tb, np.where(pb == 0xFFFFFFFF, -1, pb.astype(np.int64)), uvb, osc.shade_hits(tb, pb, uvb), "bvh", name)
    if name == "grid_zero_nonfinite":
        assert (pid < 0).all() and (ref.n == 0).all()           # the documented result: a miss


RAY_MUTANTS = {"second": ("room_random", "room_hemisphere", "house_random", "scan_random", "patho_soup"),
               "drop": tuple(n for n in NAMES if n not in ("grid_zero_nonfinite",))}


@pytest.mark.parametrize("mut", sorted(RAY_MUTANTS))
def test_tracer_mutants_are_rejected(mut):
    """the second-closest triangle for one ray per thousand; a miss for one robust hit per ten thousand rays (at least one ray of a case).  `second` applies
    where rays are sampled and a ray can have a second triangle at all (not inside the convex box; on the aimed cases the second triangle shares the edge
    and is a candidate itself: correct to accept)"""
    for name in RAY_MUTANTS[mut]:
        c = cases()[name]
        ref = c.ref()
        t, pid, uv = TC.trace_f32(c.geo, c.org, c.dir, mut=mut, seed=11)
        if mut == "drop":
            t0, p0, _ = traced(name)
            changed = np.nonzero((p0 >= 0) & (pid < 0))[0]
            if not ref.robust[changed].any():
                continue                                       # (the dropped hit was not robust: a miss is admissible there)
        assert TC.rejected(TC.check_hits, ref, t, pid, uv, None, "mutant", "%s %s" % (mut, name)), (mut, name)


SHADE_MUTANTS = ("uv_swapped", "no_flip", "wrap", "t_gt_0")


def _applies(c, ref, mut):
    """from the reference alone: does the mutated float64 radiance of some ray's only candidate leave the reference's bound?"""
    one = (ref.n == 1) & ref.robust
    if mut == "t_gt_0":
        return bool((one & ~ref.lit[:, 0] & ~ref.kink[:, 0] & (ref.L[:, 0].max(1) > ref.bL[:, 0].max(1))).any())
    one &= ref.lit[:, 0] & ~ref.kink[:, 0]
    r = np.nonzero(one)[0]
    if not r.size:
        return False
    b = np.stack([ref.c["b0"][r, 0], ref.c["b1"][r, 0], ref.c["b2"][r, 0]], 1)
    Lm, bm = TC.shade64(c.geo, ref.id[r, 0], ref.u[r, 0], ref.v[r, 0], b, mut)
    return bool((np.abs(Lm - ref.L[r, 0]) > 2 * (bm + ref.bL[r, 0])).any())


@pytest.mark.parametrize("mut", SHADE_MUTANTS)
def test_shading_mutants_are_rejected(mut):
    applied = []
    for name in NAMES:
        c = cases()[name]
        ref = c.ref()
        if not _applies(c, ref, mut):
            continue
        applied.append(name)
        t, pid, uv = traced(name)
        assert TC.rejected(TC.check_hits, ref, t, pid, uv, TC.shade_f32(c.geo, t, pid, uv, mut), "mutant", "%s %s" % (mut, name)), (mut, name)
    print(mut, "applies to", applied)
    assert len(applied) >= (1 if mut in ("t_gt_0", "wrap") else 8), applied


def test_shading_stage_on_given_records_and_the_clip_mutant():
    """query_irf's arithmetic on GIVEN hit records, barycentrics outside [0, 1] included (a watertight tracer never returns those: the clip is checked here)"""
    from texture_cases import check, rejected
    applied = {}
    for geo in (TC.golden_geo("room")[0], TC.pathological_geos()["soup"], TC.box_grid_geo(8)):
        pid, uv, t = TC.shade_records(geo)
        L, b = TC.shade64(geo, pid, uv[:, 0], uv[:, 1])
        check(TC.shade_f32(geo, t, pid, uv), L, b, "shade", geo.name)
        for mut in ("no_clip", "uv_swapped", "no_flip", "wrap"):
            Lm, bm = TC.shade64(geo, pid, uv[:, 0], uv[:, 1], mut=mut)
            if (np.abs(Lm - L) > 2 * (b + bm)).any():              # (wrap: only where a chart reaches the half texel along the texture's border)
                applied.setdefault(mut, []).append(geo.name)
                assert rejected(TC.shade_f32(geo, t, pid, uv, mut), L, b), (geo.name, mut)
    assert all(len(applied[m]) == 3 for m in ("no_clip", "uv_swapped", "no_flip")) and len(applied["wrap"]) >= 2, applied


@pytest.mark.parametrize("key", TC.CPU_IRT, ids=lambda k: "%s_%dx%d_%s%s%s" % (k[0], k[1], k[2], k[3], "_cosw" if k[4] else "", "_" + k[5] if k[5] else ""))
def test_irt_float32_estimator_is_accepted_and_mutants_rejected(key):
    from oracle import oracle as O
    c = TC.irt_case(*key)
    ref, i, N = c.ref(), c.ids, c.N
    over, multi, unsharp = ref.caps()
    print("caps %-28s overflow %d, samples with more than one outcome %.4f, texels not sharp %.3f" % (c.name, over, multi, unsharp))
    assert over == 0 and multi <= TC.CAP_MULTI and unsharp <= TC.CAP_UNSHARP
    d = O.generate_dir(c.nrm[i], N, c.mode, c.shift[i])
    t, pid, uv = TC.trace_f32(c.geo, np.repeat(c.pos[i], N, 0), d.reshape(-1, 3))
    L = TC.shade_f32(c.geo, t, pid, uv).reshape(len(i), N, 3)
    valid = np.zeros(len(c.pos), np.uint8)
    valid[i] = 1
    got = c.geo.osc().irt_generate(c.pos, c.nrm, valid, c.shift, N, c.mode, tracer="bvh", cosine_estimator=c.cosw)
    ref.check(got[i], "wave", 1, "irt_bvh", c.name)          # (the oracle accumulates in double: fewer roundings than any form allows)
    for form in ("wave", "group"):
        parts = TC.n_parts(N, form)
        ref.check(TC.estimator_f32(c.nrm[i], d, L, c.cosw, form, parts), form, parts, "irt_f32", "%s %s/%d" % (c.name, form, parts))
        for mut, applies in TC.IRT_MUTANTS.items():
            if not applies(c) or (mut == "drop_part" and parts != 32):
                continue
            bad = TC.estimator_f32(c.nrm[i], d, L, c.cosw, form, parts, mut)
            assert TC.rejected(ref.check, bad, form, parts, "mutant", "%s %s %s" % (mut, c.name, form)), (mut, c.name, form)


def test_every_irt_mutant_applies_somewhere():
    for mut, applies in TC.IRT_MUTANTS.items():
        assert any(applies(TC.irt_case(*k)) for k in TC.CPU_IRT), mut
    assert TC.n_parts(512, "group") == 32 and TC.n_parts(2048, "stream") == 32 and TC.n_parts(64, "group") == 8 and TC.n_parts(100, "group") == 1
    assert TC.n_parts(2048, "group", min_part_cells=64) == 32 and TC.n_parts(512, "group", min_part_cells=64) == 8 and TC.n_parts(512, "group", log2parts_cap=0) == 1
    assert TC.n_acc(2048, "wave") == 1 + 32 + 6 + 3 + 2 and TC.n_acc(2048, "group", 32) == 1 + 64 + 31 + 3 + 2


@pytest.mark.parametrize("key", TC.GPU_IRT, ids=lambda k: "%s_%dx%d_%s%s%s" % (k[0], k[1], k[2], k[3], "_cosw" if k[4] else "", "_" + k[5] if k[5] else ""))
def test_caps_of_the_gpu_irt_cases(key):
    c = TC.irt_case(*key)
    over, multi, unsharp = c.ref().caps()
    print("caps %-28s overflow %d, samples with more than one outcome %.4f, texels not sharp %.3f" % (c.name, over, multi, unsharp))
    assert over == 0 and multi <= TC.CAP_MULTI and unsharp <= TC.CAP_UNSHARP
    TC._IRT.pop(TC.irt_key(*key))                              # (the references are large)


def test_caps_of_the_gpu_ray_cases():
    for c in TC.ray_cases():
        over, multi = TC.ray_caps(c.ref())
        print("caps %-22s rays %6d overflow %d, rays with more than one outcome %.4f" % (c.name, c.ref().R, over, multi))
        assert over == 0
        assert c.name in AIMED or multi <= TC.CAP_MULTI
