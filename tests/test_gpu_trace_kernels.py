"""trace_core / trace_closest / trace_stream (csrc/device_common.h) and irt_kernel, irt_group_kernel, irt_stream_kernel, irt_combine_kernel, trace_shade_kernel
(csrc/kernels.hip) against the float64 reference of tests/trace_cases.py: EVERY ray by the per-ray rule (candidate, t, u, v, closest robust hit, radiance),
EVERY texel inside the sum of its samples' intervals -- never one kernel form against another.  The margins, bounds and caps are derived in trace_cases.py
and proved on the CPU by test_trace_ref_cpu.py.

MEASURED on an MI355X (151 tests, all passing; worst error / bound per family, 1.0 = the bound; every ray and every texel compared, none rejected):
    rays      15 cases, 43 k rays: room / box random + texel hemispheres, house, scan, the four pathological meshes, the closed cube aimed at shared
              vertices / edges, axis-parallel, from a face, un-normalised, zero and non-finite directions                                            0.102
    builds    TEXIR_BVH_WIDTH=2, TEXIR_UNIFORM_FLOAT=0, TEXIR_MAX_LEAF=1 / 8 on five of them                                                        0.089
    layouts   TEXIR_TEX_LAYOUT 0 .. 4 (room, texture as an RGBE file times a power of two)                                                          0.084
    irt       22 cases x TEXIR_IRT_TEXELS_PER_WAVE 0 / 1 / 64                                                                                       0.569
    irt_list  lists of 1 / 63 / 65 / 130 texels, no list                                                                                            0.569
    irt_sw    tree builds, TEXIR_IRT_REFILL 8 / 32 / 63 (irt_stream_kernel), TEXIR_IRT_LOG2PARTS=0, TEXIR_IRT_MIN_PART_CELLS=64 at N = 64 / 512 / 2048     0.569
    irt_tex   TEXIR_TEX_LAYOUT 0 .. 4 in the 64-texel form                                                                                          0.568
    spec_Ls   the lighting spec_forward_raw traces itself, 200 pixels x 16 samples                                                                  0.076
(the IrT figure is one texel of the 130-texel list at N = 64 / 65, the same in every kernel form; every other IrT case stays below 0.08.)
Caps (test_trace_ref_cpu.py, from the reference alone): no ray overflows its candidate list; samples with more than one admissible outcome at most 0.11 % of an
IrT case (cap 2 %) and 0.57 % of a sampled ray case; texels that are not sharp at most 4.3 % of a case (cap 20 %).
Time: the float64 reference of all cases takes 75 s on 8 CPU threads (the largest one, 70 texels x 2048 samples against 20 000 triangles, 27 s); the module
adds 22 s to the GPU suite on an MI355X machine that grants 16 CPUs, the references (about 15 s there) included.
"""
import numpy as np
import pytest
import torch

import trace_cases as TC

pytestmark = pytest.mark.gpu

_RAYS = {}


def ray_case(name):
    if not _RAYS:
        for c in TC.ray_cases():
            _RAYS[c.name] = c
    return _RAYS[name]


RAY_NAMES = ["room_random", "room_hemisphere", "box_random", "box_hemisphere", "house_random", "scan_random", "patho_stack", "patho_fan", "patho_soup", "patho_single",
             "grid_vertices_edges", "grid_axis_parallel", "grid_on_face", "grid_unnormalised", "grid_zero_nonfinite"]


def gpu_scene(tx, geo):
    return tx.Scene(geo.verts, geo.tris, geo.tri_uvs, geo.hdr)


def trace(sc, case):
    rad, t, pid, uv = sc.trace_shade(torch.from_numpy(case.org), torch.from_numpy(case.dir), return_hits=True)
    return t.cpu().numpy(), pid.cpu().numpy().astype(np.int64), uv.cpu().numpy(), rad.cpu().numpy()


@pytest.mark.parametrize("name", RAY_NAMES)
def test_closest_hits_per_ray(tx, name):
    c = ray_case(name)
    t, pid, uv, rad = trace(gpu_scene(tx, c.geo), c)
    TC.check_hits(c.ref(), t, pid, uv, rad, "rays", name)
    if name == "grid_zero_nonfinite":
        assert (pid == -1).all() and np.isinf(t).all() and (rad == 0).all()


BUILDS = [("TEXIR_BVH_WIDTH", "2"), ("TEXIR_UNIFORM_FLOAT", "0"), ("TEXIR_MAX_LEAF", "1"), ("TEXIR_MAX_LEAF", "8")]


@pytest.mark.parametrize("var,value", BUILDS)
@pytest.mark.parametrize("name", ["room_random", "scan_random", "patho_soup", "grid_vertices_edges", "grid_on_face"])
def test_closest_hits_per_ray_other_tree_builds(tx, monkeypatch, name, var, value):
    """binary tree, no float node copy, leaves of one and of up to eight triangles: each against the reference"""
    monkeypatch.setenv(var, value)
    c = ray_case(name)
    t, pid, uv, rad = trace(gpu_scene(tx, c.geo), c)
    TC.check_hits(c.ref(), t, pid, uv, rad, "builds", "%s %s=%s" % (name, var, value))


@pytest.mark.parametrize("layout", ["0", "1", "2", "3", "4"])
def test_hit_shader_texture_layouts(tx, monkeypatch, layout):
    """the five texture layouts of the hit shader; 3 and 4 hold 4-byte texels and need a texture that packs exactly (an RGBE file times a power of two)"""
    from texir_code_amd import synth
    base = ray_case("room_random")
    geo = TC.Geo("room_born", base.geo.verts, base.geo.tris, base.geo.tri_uvs, synth.rgbe_born(base.geo.hdr))
    c = TC.RayCase("room_born_random", geo, base.org, base.dir)
    key = "born_ref"
    if key not in _RAYS:
        _RAYS[key] = c.ref()
    monkeypatch.setenv("TEXIR_TEX_LAYOUT", layout)
    sc = gpu_scene(tx, geo)
    assert sc.texture_layout() == int(layout)
    t, pid, uv, rad = trace(sc, c)
    TC.check_hits(_RAYS[key], t, pid, uv, rad, "layouts", "layout %s" % layout)


# ---- IrT ---------------------------------------------------------------------------------------------------------------------------------------------------

def irt_run(tx, c, sc=None, ids="list", rows=None, min_part_cells=8, log2parts_cap=5, family="irt", what=""):
    """launch irt_generate on the case's listed texels (rows: a prefix of them), name the kernel form from the launcher's own decision, compare every listed
    texel with the reference; unlisted texels must stay untouched"""
    sc = gpu_scene(tx, c.geo) if sc is None else sc
    use = c.ids if rows is None else c.ids[rows]
    out = torch.full((len(c.pos), 3), 7.0, device="cuda")
    tid = torch.from_numpy(use.astype(np.int32)).cuda()
    if c.cosw:
        # the cosine estimator (pi / N) sum L over cosine-distributed directions is diffuse_irradiance(..., "cosine"): the same kernels, no id list
        from texir_code_amd import scene as S
        assert c.mode == "cosine"
        f = lambda a: torch.from_numpy(np.ascontiguousarray(a[use])).cuda()
        irr = np.full((len(c.pos), 3), 7.0, np.float32)
        irr[use] = S.diffuse_irradiance(sc, f(c.pos), f(c.nrm), f(c.shift), c.N, "cosine").cpu().numpy()
    else:
        irr = sc.irt_generate(torch.from_numpy(c.pos), torch.from_numpy(c.nrm), torch.from_numpy(c.shift), c.N, c.mode, texel_ids=tid, out=out).cpu().numpy()
    name = sc.irt_kernel_name(len(use), c.N)
    form = "wave" if name.startswith("irt_kernel") else ("stream" if "stream" in name else "group")
    parts = TC.n_parts(c.N, form, min_part_cells, log2parts_cap)
    c.ref().check(irr[use], form, parts, family, "%s %s %s/%d" % (c.name, what, form, parts), rows=rows)
    unlisted = np.ones(len(c.pos), bool)
    unlisted[use] = False
    assert (irr[unlisted] == 7.0).all()
    return form, parts


IRT_IDS = ["%s_%dx%d_%s%s%s" % (k[0], k[1], k[2], k[3], "_cosw" if k[4] else "", "_" + k[5] if k[5] else "") for k in TC.GPU_IRT]


@pytest.mark.parametrize("per_wave", ["0", "1", "64"])
@pytest.mark.parametrize("key", TC.GPU_IRT, ids=IRT_IDS)
def test_irt_per_texel(tx, monkeypatch, key, per_wave):
    """N in {1, 2, 63, 64, 65, 100, 128, 512, 2048}, modes uniform and cosine, the cosine estimator, normals on both sides of |n.x| = 0.99 and longer than 1,
    shifts 0 and next to 1 -- the automatic form, one texel per wave and 64 texels per wave"""
    monkeypatch.setenv("TEXIR_IRT_TEXELS_PER_WAVE", per_wave)
    form, _ = irt_run(tx, TC.irt_case(*key), what="per_wave=%s" % per_wave)
    assert form == ("group" if per_wave == "64" else "wave")


@pytest.mark.parametrize("n", [1, 63, 65, 130])
@pytest.mark.parametrize("per_wave", ["1", "64"])
def test_irt_ragged_lists(tx, monkeypatch, n, per_wave):
    monkeypatch.setenv("TEXIR_IRT_TEXELS_PER_WAVE", per_wave)
    irt_run(tx, TC.irt_case("room", 130, 64, "uniform"), rows=slice(0, n), family="irt_list", what="first %d per_wave=%s" % (n, per_wave))


def test_irt_without_id_list(tx):
    """no list: every texel; an invalid texel (zero normal: zero direction, a miss) is exactly zero"""
    c = TC.irt_case("box", 642, 64, "uniform")
    _, gb = TC.golden_geo("box")
    sc = gpu_scene(tx, c.geo)
    irr = sc.irt_generate(torch.from_numpy(c.pos), torch.from_numpy(c.nrm), torch.from_numpy(c.shift), 64, "uniform").cpu().numpy()
    form = "wave" if sc.irt_kernel_name(len(c.pos), 64).startswith("irt_kernel") else "group"
    c.ref().check(irr[c.ids], form, TC.n_parts(64, form), "irt_list", "box, no id list")
    invalid = gb["valid"].reshape(-1) == 0
    assert invalid.sum() == len(c.pos) - len(c.ids) and (irr[invalid] == 0).all()


def test_irt_cosine_estimator_listed_texels_equal_all(tx, monkeypatch):
    """the cosine estimator through irt_combine_kernel (64-texel form: 8 parts at N = 64), which the uniform one reaches with an id list in
    test_irt_ragged_lists: diffuse_irradiance takes no list, so 65 of 130 texels are handed over as their own rows and must get, bit for bit, what they
    get in the call over all 130 (a texel's sum depends on the texel and N alone)"""
    from texir_code_amd import scene as S
    monkeypatch.setenv("TEXIR_IRT_TEXELS_PER_WAVE", "64")
    c = TC.irt_case("room", 130, 64, "uniform")
    sc = gpu_scene(tx, c.geo)
    assert len(c.ids) == 130 and sc.irt_kernel_name(65, 64).startswith("irt_group_kernel") and TC.n_parts(64, "group") == 8
    listed = np.arange(0, 130, 2)
    f = lambda a, rows: torch.from_numpy(np.ascontiguousarray(a[c.ids][rows])).cuda()
    run = lambda rows: S.diffuse_irradiance(sc, f(c.pos, rows), f(c.nrm, rows), f(c.shift, rows), 64, "cosine").cpu().numpy()
    every, some = run(np.arange(130)), run(listed)
    assert some.shape == (65, 3) and np.isfinite(every).all() and (every > 0).any()
    assert (some.view(np.uint32) == every[listed].view(np.uint32)).all()


SWITCHES = [({"TEXIR_BVH_WIDTH": "2"}, {}), ({"TEXIR_UNIFORM_FLOAT": "0"}, {}), ({"TEXIR_MAX_LEAF": "1"}, {}), ({"TEXIR_MAX_LEAF": "8"}, {}),
            ({"TEXIR_IRT_REFILL": "8"}, {}), ({"TEXIR_IRT_REFILL": "32"}, {}), ({"TEXIR_IRT_REFILL": "63"}, {}),
            ({"TEXIR_IRT_LOG2PARTS": "0"}, {"log2parts_cap": 0}), ({"TEXIR_IRT_MIN_PART_CELLS": "64"}, {"min_part_cells": 64}),
            ({"TEXIR_IRT_REFILL": "32", "TEXIR_IRT_MIN_PART_CELLS": "64"}, {"min_part_cells": 64})]


@pytest.mark.parametrize("env,plan", SWITCHES, ids=["+".join("%s=%s" % kv for kv in e.items()).replace("TEXIR_", "") for e, _ in SWITCHES])
@pytest.mark.parametrize("key", [("room", 130, 64, "uniform", False, None), ("room", 70, 512, "uniform", False, None), ("room", 70, 2048, "uniform", False, None)],
                         ids=["N64", "N512", "N2048"])
def test_irt_switches(tx, monkeypatch, key, env, plan):
    """tree builds, the stream kernel (refill at 8 / 32 / 63 idle lanes), one part and parts of at least 64 passes -- all in the 64-texel form, where they act"""
    monkeypatch.setenv("TEXIR_IRT_TEXELS_PER_WAVE", "64")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    form, parts = irt_run(tx, TC.irt_case(*key), family="irt_sw", what=" ".join("%s=%s" % kv for kv in env.items()).replace("TEXIR_", ""), **plan)
    if "TEXIR_IRT_REFILL" in env and parts > 1:
        assert form == "stream"
    if "TEXIR_BVH_WIDTH" in env:
        assert form == "wave"                                  # (a binary tree has the one-texel form only)


@pytest.mark.parametrize("layout", ["0", "1", "2", "3", "4"])
def test_irt_texture_layouts(tx, monkeypatch, layout):
    from texir_code_amd import synth
    base = TC.irt_case("room", 130, 64, "uniform")
    if "born" not in TC._IRT:
        geo = TC.Geo("room_born", base.geo.verts, base.geo.tris, base.geo.tri_uvs, synth.rgbe_born(base.geo.hdr))
        c = TC.IrtCase("room", base.ids, 64, "uniform")
        c.geo, c.name = geo, "room_born_130x64_uniform"
        TC._IRT["born"] = c
    c = TC._IRT["born"]
    monkeypatch.setenv("TEXIR_TEX_LAYOUT", layout)
    monkeypatch.setenv("TEXIR_IRT_TEXELS_PER_WAVE", "64")
    sc = gpu_scene(tx, c.geo)
    assert sc.texture_layout() == int(layout)
    irt_run(tx, c, sc=sc, family="irt_tex", what="layout %s" % layout)


def test_specular_lighting_per_sample(tx):
    """the lighting spec_forward_raw traces for itself (Ls): per sample by the per-ray rule, the direction l and its bound from spec_cases"""
    import spec_cases as SC
    from texir_code_amd import scene as S
    geo, gb = TC.golden_geo("room")
    rng = np.random.default_rng(5)
    v = np.argwhere(gb["valid"].reshape(-1) > 0)[:, 0][::13][:200]
    P, Sn = len(v), 16
    n, pts = gb["nrm"].reshape(-1, 3)[v], gb["pos"].reshape(-1, 3)[v]
    r = rng.uniform(0.05, 0.8, P).astype(np.float32)
    shift = rng.uniform(0, 1, (P, 2)).astype(np.float32)
    cam = np.array([4.0, 1.5, 3.0], np.float32)
    names = ("l0", "l1", "l2")
    ref = SC.reference(SC.sample_inputs(n, r, pts, cam, shift, Sn), 1e-14, "spec", names)
    assert not ref.left.any()
    vi, si = np.nonzero(ref.adm)
    d = np.stack([ref.val[k][vi, si] for k in names], 1)
    bd = np.stack([ref.bnd[k][vi, si] for k in names], 1)
    rays = TC.RayRef(geo, pts.astype(np.float64)[si // Sn], d, bd)
    assert not rays.overflow.any()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    alb, irr = t(rng.uniform(0, 1, (P, 3))), t(rng.uniform(0, 3, (P, 3)))
    _, Ls, _ = S.spec_forward_raw(gpu_scene(tx, geo), t(n), alb, t(r), t(pts), irr, t(cam), t(shift), Sn)
    TC.check_radiance(rays, Ls.cpu().numpy().reshape(-1, 3), "spec_Ls", "room 200 x 16", sample_of=si)
