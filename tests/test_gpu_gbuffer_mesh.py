"""gbuffer_mesh_kernel (csrc/gbuffermesh.hip; texir_gbuffer_cast_mesh; gbuffer.cast_gbuffer(occluders=...)) against the float64 reference of
tests/gbuffer_mesh_cases.py: EVERY pixel of every case inside the reference -- the surface and the triangle admissible, position and normal of an instance pixel
inside bounds derived from the reference alone, uv, uv_da, mask, tri_id and inst_id of an instance pixel exact, the room's pixels by gbuffer_cases' own check --
and the rule's exact statements bit for bit: J = 0, unseen instances, a NaN matrix and an exact tie with the scene give texir_gbuffer_cast's bits; the lower
index wins an exact tie; the prefilter, the form of the poses, a replayed graph and a second run change no bit.  The bounds and caps are derived in
gbuffer_mesh_cases.py and proved on the CPU by test_gbuffer_mesh_ref_cpu.py; they were fixed before the first GPU run and not adjusted afterwards.

Cases: the closed 192-triangle cube from its centre and from 0.06 off a wall at c = 8 and 17 with a box under rotation and non-uniform scale, an icosphere, one
occluder under two poses, a mirrored pose, two interpenetrating instances, a cube the wall cuts beside one wholly behind the wall, an icosphere around the eye and
eight instances; the golden room with the table at c = 16; c = 296 with an icosphere in view of the grid-stride loop's second trip.  Every case runs with flip_v
0 and 1, on a fresh scene and after set_corner_normals.

MEASURED on an MI355X (129 tests, all passing, 4.5 s; worst error / bound per output, 1.0 = the bound; every pixel compared, none rejected):
    output                            34 cases x 2 normal modes x 2 flip_v
    position, instance pixels         0.118  (stride_c296: the instance 0.027 from the eye)
    normal, instance pixels           0.017  (twice_graze_c17, the instance under rotation and non-uniform scale)
    position, room pixels             0.049  (room_table_c16)
    uv                                0.061  (room_table_c16, flip_v = 1)
    uv_da                             0.037  (stride_c296)
    normal, room, interpolated        0.014  (room_table_c16)
    normal, room, geometric           0.047  (room_table_c16)
    surface and triangle              every (inst_id, tri_id) an admissible outcome; uv, uv_da, mask of every instance pixel exact
Neither the kernel nor a bound was changed after the first run.  One test's own construction was: the exact tie with the scene was first built from
Scene.occluder(room mesh), whose dummy uvs let the builder pair triangles into other quad records than the room's -- the same surface, but a t that
differs in the last bit on a few pixels, which is no tie.  The room's mesh with the room's own uvs gives the same tree, and then every pixel ties and the
scene wins, with the prefilter on and off.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import gbuffer_cases as GC
import gbuffer_mesh_cases as GM
import irt_shadow_mesh_cases as MC

pytestmark = pytest.mark.gpu

ROOM_KEYS = ("position", "normal", "mask", "uv", "uv_da", "tri_id")
EXACT = ("mask", "tri_id", "inst_id", "uv", "uv_da")


def gpu_scene(tx, geo):
    return tx.Scene(geo.verts, geo.tris, geo.tri_uvs, geo.hdr)


def occluders_of(tx, case):
    return [tx.Scene.occluder(g.verts, g.tris) for g in case.geos()]


def cast(sc, case, occ, flip_v, poses=None, inst=None, prefilter=True):
    from texir_code_amd import gbuffer as GB
    out = GB.cast_gbuffer(sc, torch.from_numpy(case.mvp), case.c, flip_v=bool(flip_v), occluders=occ, instances=case.inst if inst is None else inst,
                          poses=case.poses if poses is None else poses, prefilter=prefilter)
    c = case.c
    assert out["inst_id"].shape == (6, c, c) and out["inst_id"].dtype == torch.int32 and out["position"].shape == (6, c, c, 3)
    return {k: out[k].cpu().numpy() for k in GM.KEYS}


def plain(sc, case, flip_v):
    from texir_code_amd import gbuffer as GB
    out = GB.cast_gbuffer(sc, torch.from_numpy(case.mvp), case.c, flip_v=bool(flip_v))
    assert "inst_id" not in out
    return {k: out[k].cpu().numpy() for k in ROOM_KEYS}


def same_bits(a, b, keys=GM.KEYS):
    return [k for k in keys if a[k].tobytes() != b[k].tobytes()]


def is_plain(got, want):
    """`got` holds texir_gbuffer_cast's bits and inst_id = -1 everywhere"""
    return same_bits(got, want, ROOM_KEYS) == [] and bool((got["inst_id"] == -1).all())


_RUNS = {}


def runs(tx, name):
    """every cast of a case, made once and shared by the tests below: (normals, flip_v, prefilter) -> outputs; normals 0: a fresh scene, 1: after
    set_corner_normals"""
    if name not in _RUNS:
        from texir_code_amd import gbuffer as GB
        case = GM.case(name)
        sc, occ = gpu_scene(tx, case.geo), occluders_of(tx, case)
        r = {}
        for normals in (0, 1):
            if normals:
                GB.set_corner_normals(sc, GC.corner_normals(case.geo))
            for flip_v in (0, 1):
                r[(normals, flip_v, True)] = cast(sc, case, occ, flip_v)
                r[(normals, flip_v, False)] = cast(sc, case, occ, flip_v, prefilter=False)
        r["again"] = cast(sc, case, occ, 1)
        _RUNS[name] = r
    return _RUNS[name]


# ---- 1. every pixel inside the float64 reference ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", GM.NAMES)
def test_every_pixel_inside_the_reference(tx, name):
    case = GM.case(name)
    r = runs(tx, name)
    if name == "stride_c296":
        P = 6 * case.c * case.c
        pix = case.ref().g.pix
        assert P > GC.STRIDE_START and (pix >= GC.STRIDE_START).sum() == P - GC.STRIDE_START        # every pixel of the second trip is compared
        assert (r[(0, 0, True)]["inst_id"].reshape(-1)[GC.STRIDE_START:] >= 0).sum() >= 0.05 * (P - GC.STRIDE_START)
    cn = GC.corner_normals(case.geo)
    for normals in (0, 1):
        for flip_v in (0, 1):
            GM.check(case, r[(normals, flip_v, True)], cn if normals else None, flip_v, "gbm", "interpolated" if normals else "geometric")
    if not case.degenerate:
        share = float((r[(0, 0, True)]["inst_id"].reshape(-1)[case.ref().g.pix] >= 0).mean())
        assert share >= GM.CAP_SHARE                                                               # the instance is really drawn


# ---- 2. what must be texir_gbuffer_cast's bits ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["box_graze_c8", "box_centre_c17", "room_table_c16"])
def test_nothing_drawn_gives_the_plain_gbuffer_bit_for_bit(tx, name):
    from texir_code_amd import gbuffer as GB
    case = GM.case(name)
    sc, occ = gpu_scene(tx, case.geo), occluders_of(tx, case)
    # the room's own mesh as an occluder, built with the room's own uvs: the builder pairs triangles into quad records across edges without a uv seam, so
    # Scene.occluder's dummy uvs would give other records, whose t differs from the room's in the last bit (the corners enter the sum in another order) --
    # an equal surface, not an exact tie.  With the same uvs the two trees are the same and every pixel is an exact tie.
    own = gpu_scene(tx, case.geo)
    eye = np.eye(3, 4)[None]
    far = np.stack([MC.pose((50.0 + 3.0 * j, -40.0, 60.0), (1, 2, 3), 20.0 * j, 0.7) for j in range(case.J)])      # wholly outside the room
    seen = cast(sc, case, occ, 1)
    assert (seen["inst_id"] >= 0).any()
    nan = torch.from_numpy(case.w2o.copy()).cuda()
    nan[:, 5] = float("nan")
    for normals in (0, 1):
        if normals:
            GB.set_corner_normals(sc, GC.corner_normals(case.geo))
        for flip_v in (0, 1):
            want = plain(sc, case, flip_v)
            what = (name, normals, flip_v)
            assert is_plain(cast(sc, case, [], flip_v, poses=np.zeros((0, 3, 4)), inst=[]), want), ("J = 0, Q = 0",) + what
            assert is_plain(cast(sc, case, occ, flip_v, poses=np.zeros((0, 3, 4)), inst=[]), want), ("J = 0",) + what
            for pf in (True, False):
                assert is_plain(cast(sc, case, occ, flip_v, poses=far, prefilter=pf), want), ("instances outside", pf) + what
                assert is_plain(cast(sc, case, occ, flip_v, poses=nan, prefilter=pf), want), ("a NaN in every matrix", pf) + what
                assert is_plain(cast(sc, case, [own], flip_v, poses=eye, inst=[0], prefilter=pf), want), ("the room's own mesh: a tie on every pixel", pf) + what


def test_one_nan_matrix_removes_that_instance_alone(tx):
    case = GM.case("twice_graze_c8")
    sc, occ = gpu_scene(tx, case.geo), occluders_of(tx, case)
    both = cast(sc, case, occ, 1)
    assert set(np.unique(both["inst_id"])) == {-1, 0, 1}
    w = torch.from_numpy(case.w2o.copy()).cuda()
    w[0, 11] = float("nan")
    got = cast(sc, case, occ, 1, poses=w)
    alone = cast(sc, case, occ, 1, poses=case.poses[1:], inst=case.inst[1:])
    assert set(np.unique(got["inst_id"])) == {-1, 1}
    alone["inst_id"] = np.where(alone["inst_id"] == 0, 1, alone["inst_id"])         # (the same object, one index lower)
    assert same_bits(got, alone) == []


# ---- 3. the lower index wins an exact tie ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["ico_graze_c17", "mirror_centre_c8"])
def test_the_same_instance_twice_reports_the_lower_index(tx, name):
    case = GM.case(name)
    sc, occ = gpu_scene(tx, case.geo), occluders_of(tx, case)
    once = cast(sc, case, occ, 0)
    for pf in (True, False):
        twice = cast(sc, case, occ, 0, poses=np.concatenate([case.poses, case.poses]), inst=case.inst + case.inst, prefilter=pf)
        assert (twice["inst_id"] >= 0).any() and twice["inst_id"].max() == 0
        assert same_bits(once, twice) == []


# ---- 4. the prefilter changes no bit; 8. two runs are bit-identical ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", GM.NAMES)
def test_prefilter_off_and_a_second_run_give_the_same_bits(tx, name):
    r = runs(tx, name)
    for normals in (0, 1):
        for flip_v in (0, 1):
            assert same_bits(r[(normals, flip_v, True)], r[(normals, flip_v, False)]) == [], (name, normals, flip_v)
    assert same_bits(r[(1, 1, True)], r["again"]) == []


# ---- 5. the float32 restatement ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", GM.NAMES)
def test_agreement_with_the_float32_restatement_where_the_outcome_is_single(tx, name):
    case = GM.case(name)
    ref = case.ref()
    n_out = sum(a.sum(1) for a in ref.adm) + ref.bg_ok                               # every admissible (surface, triangle), and the background
    single = n_out == 1
    assert single.mean() > 0.5 or case.base.aimed
    pix = ref.g.pix[single]
    P = 6 * case.c * case.c
    r = runs(tx, name)
    for flip_v in (0, 1):
        want = GM.gbuffer_mesh_f32(case, None, flip_v)
        got = r[(0, flip_v, True)]
        for k in ("mask", "tri_id", "inst_id"):
            a, b = np.asarray(got[k]).reshape(P)[pix], np.asarray(want[k]).reshape(P)[pix]
            assert (a == b).all(), "%s: %s differs from the restatement on %d of %d single-outcome pixels, first pixel %d" % (name, k, int((a != b).sum()), len(pix),
                                                                                                                        pix[np.nonzero(a != b)[0][0]])
        on = pix[np.asarray(want["inst_id"]).reshape(P)[pix] >= 0]
        for k in ("uv", "uv_da"):
            assert (np.asarray(got[k]).reshape(P, -1)[on] == 0).all() and (np.asarray(want[k]).reshape(P, -1)[on] == 0).all()


# ---- 6. host poses, device matrices, a replayed graph --------------------------------------------------------------------------------------------------------------------

def test_device_matrices_and_a_replayed_graph_see_the_moved_object(tx):
    from texir_code_amd import _lib
    case, moved = GM.case("box_graze_c17"), GM.case("ico_graze_c17")
    sc = gpu_scene(tx, case.geo)
    occ = [tx.Scene.occluder(g.verts, g.tris) for g in case.geos()]
    host = cast(sc, case, occ, 1)
    w2o = torch.from_numpy(case.w2o.copy()).cuda()
    assert same_bits(host, cast(sc, case, occ, 1, poses=w2o)) == [], "host poses and the device matrix form"
    other = torch.from_numpy(moved.w2o.copy()).cuda()                                # (another pose of the same box)
    fresh_other = cast(sc, case, occ, 1, poses=other)
    assert same_bits(host, fresh_other) != []
    # a graph recorded once on caller-owned buffers; the matrix lives on the device and is overwritten between replays
    L = _lib.lib()
    P = 6 * case.c * case.c
    bufs = [torch.full((P, k), 7.25, device="cuda") for k in (3, 3, 1, 2, 4)]
    tri, iid = torch.full((P,), 77, device="cuda", dtype=torch.int32), torch.full((P,), 77, device="cuda", dtype=torch.int32)
    handles = (C.c_void_p * len(occ))(*[o.h for o in occ])
    inst = np.array(case.inst, np.int32)
    mvp = np.ascontiguousarray(case.mvp, np.float32)
    live = w2o.clone()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):                                       # the single call on one stream: no parallel branches
            _lib.check(L.texir_gbuffer_cast_mesh(sc.h, _lib.ptr(mvp), case.c, 1, C.cast(handles, C.c_void_p), len(occ), _lib.ptr(inst), _lib.ptr(live), case.J, 0,
                                                 *[_lib.ptr(b) for b in bufs], _lib.ptr(tri), _lib.ptr(iid), _lib.stream_ptr()))
    torch.cuda.current_stream().wait_stream(side)

    def replayed():
        g.replay()
        torch.cuda.synchronize()
        out = dict(zip(("position", "normal", "mask", "uv", "uv_da"), [b.cpu().numpy() for b in bufs]))
        out["tri_id"], out["inst_id"] = tri.cpu().numpy(), iid.cpu().numpy()
        return out
    assert same_bits(replayed(), host) == [], "the replay with the recorded matrix"
    live.copy_(other)
    assert same_bits(replayed(), fresh_other) == [], "the replay after the matrix was overwritten"


# ---- 7. refused arguments ---------------------------------------------------------------------------------------------------------------------------------------------------

REFUSED = ("Q=9", "J=9", "Q=-1", "J=-1", "inst_obj names no occluder", "inst_obj null", "occluders null", "an occluder null", "matrices null", "scene null", "mvp null",
           "pos null", "inst_id null", "c=0", "c=16385", "singular", "affine")


@pytest.mark.parametrize("which", REFUSED)
def test_refused_arguments_return_invalid_and_write_nothing(tx, which):
    from texir_code_amd import _lib
    case = GM.case("box_graze_c8")
    sc, occ = gpu_scene(tx, case.geo), occluders_of(tx, case)
    L = _lib.lib()
    P = 6 * case.c * case.c
    fill = 7.25
    bufs = [torch.full((P, k), fill, device="cuda") for k in (3, 3, 1, 2, 4)]
    tri, iid = torch.full((P,), 77, device="cuda", dtype=torch.int32), torch.full((P,), 77, device="cuda", dtype=torch.int32)
    handles = (C.c_void_p * 9)(*([occ[0].h] * 9))
    if which == "an occluder null":
        handles[0] = None
    inst = np.array({"inst_obj names no occluder": [1]}.get(which, case.inst) * (9 if which == "J=9" else 1), np.int32)
    w2o = torch.from_numpy(np.tile(case.w2o, (9, 1))).cuda()
    Q = {"Q=9": 9, "Q=-1": -1}.get(which, 1)
    J = {"J=9": 9, "J=-1": -1}.get(which, 1)
    c = {"c=0": 0, "c=16385": 16385}.get(which, case.c)
    mvp = np.ascontiguousarray(GC.bad_mvps().get(which, case.mvp), np.float32)
    outs = [_lib.ptr(b) for b in bufs] + [_lib.ptr(tri), _lib.ptr(iid)]
    if which == "pos null":
        outs[0] = None
    if which == "inst_id null":
        outs[6] = None
    rc = L.texir_gbuffer_cast_mesh(None if which == "scene null" else sc.h, None if which == "mvp null" else _lib.ptr(mvp), c, 1,
                                   None if which == "occluders null" else C.cast(handles, C.c_void_p), Q, None if which == "inst_obj null" else _lib.ptr(inst),
                                   None if which == "matrices null" else _lib.ptr(w2o), J, 0, *outs, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1, (which, rc)                                                   # TEXIR_ERR_INVALID (include/texir_hip.h)
    assert L.texir_last_error().decode().startswith("texir_gbuffer_cast_mesh: ")
    assert all(bool((b == fill).all()) for b in bufs) and bool((tri == 77).all()) and bool((iid == 77).all())
    # the scene is still good for a valid call
    GM.check(case, cast(sc, case, occ, 0), None, 0, "gbm", "after a refused call (%s)" % which)


def test_python_surface_refuses_a_singular_pose_and_a_wrong_device_form(tx):
    case = GM.case("box_graze_c8")
    sc, occ = gpu_scene(tx, case.geo), occluders_of(tx, case)
    with pytest.raises(ValueError, match="singular"):
        cast(sc, case, occ, 0, poses=np.zeros((1, 3, 4)))
    with pytest.raises(ValueError, match="device poses"):
        cast(sc, case, occ, 0, poses=torch.zeros(1, 3, 4, device="cuda"))


def test_a_singular_finite_matrix_completes(tx):
    """the caller's error: the outputs of the pixels it touches are unspecified, the call must complete and a valid call after it is good"""
    case = GM.case("box_graze_c8")
    sc, occ = gpu_scene(tx, case.geo), occluders_of(tx, case)
    w = torch.from_numpy(case.w2o.copy()).cuda()
    w[0, 4:8] = w[0, 0:4]                                                            # two equal rows
    out = cast(sc, case, occ, 0, poses=w)
    assert out["inst_id"].min() >= -1 and out["inst_id"].max() <= 0
    GM.check(case, cast(sc, case, occ, 0), None, 0, "gbm", "after a singular matrix")


# ---- 9. the evaluation model -------------------------------------------------------------------------------------------------------------------------------------------------

def test_evaluation_model_draws_the_objects(tx, tmp_path):
    import json
    from texir_code_amd import cameras, gbuffer as GB, irtlight
    from texir_code_amd.tester import lit_model as LIT, test_model as TM
    import light_cases as LC
    geo, pos, nrm, shift, v, lo, hi = LC.room_inputs()
    ext, ctr = hi - lo, (hi + lo) / 2
    a, b = [0.3 * ext[0], 0, 0], [0, 0, 0.3 * ext[2]]
    js = tmp_path / "lights.json"
    js.write_text(json.dumps({"lights": [{"kind": "quad", "o": [ctr[0] - a[0] / 2, hi[1] - 0.15 * ext[1], ctr[2] - b[2] / 2], "a": a, "b": b, "colour": [20, 18, 15]}]}))
    tg = MC.occluder("table")
    obj = tmp_path / "table.obj"
    obj.write_text("".join("v %r %r %r\n" % tuple(float(x) for x in q) for q in tg.verts) + "".join("f %d %d %d\n" % tuple(int(i) + 1 for i in t) for t in tg.tris))
    spec = [{"obj": str(obj), "pose": {"translate": [float(ctr[0]), float(lo[1]), float(ctr[2])], "rotate_deg": [0, 20, 0], "scale": 2.0}}]
    eye = np.array([ctr[0] - 0.25 * ext[0], lo[1] + 0.8 * ext[1], ctr[2]], np.float32)   # above the table top, off its end: the table covers 6.5 % of the view
    E = np.eye(4, dtype=np.float32)
    E[:3, 3] = eye
    mvp = cameras.cube_mvps(E)[0]
    cam = torch.from_numpy(eye)
    rng = np.random.default_rng(23)
    H = 32

    def model(**keys):
        m = LIT.MaterialModel.__new__(LIT.MaterialModel)
        torch.nn.Module.__init__(m)
        m.scene = tx.Scene(geo.verts, geo.tris, geo.tri_uvs, geo.hdr)
        m.device, m.sample_l, m.sample_type, m.relighting = m.scene.device, [16, 16], ["uniform", "importance"], False
        m.cube_res, m._gb_cache, m.max_mip_level = 8, {}, 2
        r = np.random.default_rng(29)
        m.materials_a = torch.from_numpy(r.random((H, H, 3), dtype=np.float32)).cuda()
        m.materials_r = torch.from_numpy(0.1 + 0.6 * r.random((H, H, 1), dtype=np.float32)).cuda()
        m.irrt = torch.from_numpy(r.random((H, H, 3), dtype=np.float32)).cuda()
        m.texture_seg = torch.zeros((H, H, 1)).cuda()
        m.test_lights, m.light_samples = LIT.load_test_lights(str(js), m.device), 32
        m.test_objects = LIT.load_test_objects(spec, m.test_lights, m.device)
        m.spec_shadows = False
        for k, val in keys.items():
            setattr(m, k, val)
        return m
    # off: forward / render are what they are today (the attribute absent, as in a model built before this key, and false)
    off = model()
    torch.manual_seed(5)
    want_off = off.forward(mvp, 0, cam, editing=False)
    state_off = torch.get_rng_state()
    off2 = model(draw_objects=False)
    torch.manual_seed(5)
    got_off = off2.forward(mvp, 0, cam, editing=False)
    assert sorted(got_off) == sorted(want_off) and "inst_id" not in got_off
    for k in want_off:
        assert torch.equal(got_off[k], want_off[k]), k
    # on
    mats = (np.array([[0.7, 0.3, 0.2]], np.float32), np.array([0.35], np.float32))
    on = model(draw_objects=True, object_samples=64, object_albedo=torch.from_numpy(mats[0]).cuda(), object_roughness=torch.from_numpy(mats[1]).cuda())
    torch.manual_seed(5)
    res = on.forward(mvp, 0, cam, editing=False)
    assert torch.equal(torch.get_rng_state(), state_off), "drawing the objects drew from the CPU generator"
    gb = GB.cast_gbuffer(on.scene, mvp, 8, flip_v=True, **on.test_objects)
    inst = gb["inst_id"]
    assert torch.equal(res["inst_id"], inst) and torch.equal(res["empty_mask"], gb["mask"])
    obj_px = inst.reshape(-1) >= 0
    assert 0.05 < float(obj_px.float().mean()) < 0.9 and bool((gb["mask"].reshape(-1)[obj_px] == 1).all())
    # rgb = render() of the substituted inputs, assembled here from the direct calls
    from texir_code_amd.texture import texture as tex_fetch
    albedo = tex_fetch(on.materials_a, gb["uv"], gb["uv_da"], "linear-mipmap-linear", 2)
    rough = tex_fetch(on.materials_r, gb["uv"], gb["uv_da"], "linear-mipmap-linear", 2)
    irr = tex_fetch(on.irrt, gb["uv"], gb["uv_da"], "linear-mipmap-linear", 2)
    normal, points = gb["normal"], gb["position"] + 1e-2 * gb["normal"]
    P = 384
    ids = torch.nonzero(obj_px)[:, 0].to(torch.int32)
    shift_o = torch.rand(P, 2, generator=torch.Generator().manual_seed(LIT.OBJECT_SEED)).cuda()
    flat = (points.reshape(P, 3).contiguous(), normal.reshape(P, 3).contiguous())
    Eo = on.scene.irt_generate(*flat, shift_o, 64, texel_ids=ids)
    lost = on.scene.irt_shadow_mesh(*flat, shift_o, 64, sets=[[0]], texel_ids=ids, **on.test_objects)[0]
    alb2, rgh2, irr2 = albedo.reshape(P, 3).clone(), rough.reshape(P).clone(), irr.reshape(P, 3).clone()
    alb2[obj_px], rgh2[obj_px] = torch.from_numpy(mats[0]).cuda()[0], 0.35
    irr2[obj_px] = torch.clamp(Eo[obj_px] - lost[obj_px], min=0.0)
    sub = model()                                                                    # (a model without the key: its render() is today's)
    torch.manual_seed(5)
    want = sub.render(normal, alb2.reshape(albedo.shape), rgh2.reshape(rough.shape), points, cam.cuda(), irr2.reshape(irr.shape))
    assert torch.equal(res["rgb"], want["rgb"]) and torch.equal(res["albedo"], want["albedo"])
    room_px = ~obj_px
    assert torch.equal(res["rgb"].reshape(P, 3)[room_px], want["rgb"].reshape(P, 3)[room_px])
    assert bool((res["albedo"].reshape(P, 3)[obj_px] == torch.from_numpy(mats[0]).cuda()[0]).all())
    assert torch.isfinite(res["rgb"]).all()
    # the object is lit by the lamp and shadows the floor under it
    torch.manual_seed(5)
    shift_s = torch.rand(P, 1, 2).reshape(P, 2).cuda()
    records, _ = on.test_lights
    F = on.scene.irt_lights(*flat, shift_s, records, 32, **on.test_objects)[0]
    top = obj_px & (normal.reshape(P, 3)[:, 1] > 0.9)
    assert bool(top.any()) and float(F[top].max()) > 0, "no light on the table top"
    plain_gb = GB.cast_gbuffer(on.scene, mvp, 8, flip_v=True)
    pf = (plain_gb["position"] + 1e-2 * plain_gb["normal"]).reshape(P, 3).contiguous(), plain_gb["normal"].reshape(P, 3).contiguous()
    F_with = on.scene.irt_lights(*pf, shift_s, records, 32, **on.test_objects)[0]
    F_without = on.scene.irt_lights(*pf, shift_s, records, 32)[0]
    under = obj_px & (plain_gb["normal"].reshape(P, 3)[:, 1] > 0.9) & (plain_gb["position"].reshape(P, 3)[:, 1] < lo[1] + 0.05 * ext[1])   # the floor behind the table's pixels
    assert bool(under.any()) and bool((F_with[under] <= F_without[under]).all()) and float(F_with[under].sum()) < float(F_without[under].sum())
