"""The checker of the instanced cube G-buffer proved WITHOUT a GPU (tests/gbuffer_mesh_cases.py holds the reference, the bounds and the rules), and the host side
of the feature: irtobject.materials, the evaluation model's new conf keys, and the arguments gbuffer.cast_gbuffer refuses before it loads the library.

  * the caps of gbuffer_mesh_cases hold for every case of the GPU module: no candidate list overflows, at most 2 % of a case's pixels have admissible outcomes
    on more than one surface, every case not marked degenerate shows an instance alone and the room alone on at least 5 % of its pixels each;
  * gbuffer_mesh_f32, the float32 restatement of the header's rule, passes the checker on every case, both flip_v values, geometric and interpolated room normals;
  * every mutant of the restatement is rejected on at least one case.

Measured (the reference alone, 34 cases): no list overflows; more than one surface on at most 0.29 % of a case's pixels; an instance alone on 6.2 % (the cube the
wall cuts, from the centre) to 17 % of the pixels of a case that is not degenerate, 56 % to 100 % with the eye inside the instance; the room alone on 83 % to 94 %
(43 % with the eye inside an instance that pokes through the wall); the nearest instance 0.027 from the eye (the stride case).  The restatement's worst error /
bound on instance pixels: position 0.12, normal 0.017.
"""
import json

import numpy as np
import pytest

import gbuffer_cases as GC
import gbuffer_mesh_cases as GM
import trace_cases as TC


def test_case_names_are_complete():
    assert len(set(GM.NAMES)) == len(GM.NAMES) == 34
    for kind in GM.KINDS:
        assert sorted(n for n in GM.NAMES if n.startswith(kind + "_")) == sorted("%s_%s_c%d" % (kind, e, c) for e in ("centre", "graze") for c in (8, 17))
    assert set(GM.MUTANT_CASES) == set(GM.MUTANTS) and set(GM.MUTANT_CASES.values()) <= set(GM.NAMES)


@pytest.mark.parametrize("name", GM.NAMES)
def test_caps(name):
    case = GM.case(name)
    overflow, multi, inst_only, room_only, d_inst = case.ref().caps()
    print("caps %-22s overflow %d, more than one surface %.4f, an instance alone %.4f, the room alone %.4f, nearest instance %.4f" % (name, overflow, multi, inst_only,
                                                                                                                             room_only, d_inst))
    assert overflow == 0
    assert multi <= GM.CAP_MULTI
    assert d_inst >= GM.D_INST_MIN
    if not case.degenerate:
        assert inst_only >= GM.CAP_SHARE and room_only >= GM.CAP_SHARE
    if name == "stride_c296":
        second = case.ref().g.pix >= GC.STRIDE_START
        assert (case.ref().surf_ok[1] & second).sum() >= 0.05 * second.sum()        # the instance is in view of the second trip itself
    if name.startswith("mirror"):
        assert np.linalg.det(case.poses[0][:, :3]) < 0
    if name.startswith("eight"):
        assert case.J == 8 and all(case.ref().surf_ok[1 + j].any() for j in range(8))   # every one of the eight is seen somewhere


@pytest.mark.parametrize("flip_v", [0, 1])
@pytest.mark.parametrize("name", GM.NAMES)
def test_restatement_inside_every_bound(name, flip_v):
    case = GM.case(name)
    cn = GC.corner_normals(case.geo) if flip_v else None                            # (flip_v 0 with geometric, 1 with interpolated room normals)
    worst = GM.check(case, GM.gbuffer_mesh_f32(case, cn, flip_v), cn, flip_v, "gbm_f32")
    assert all(w < 1 for w in worst.values())


@pytest.mark.parametrize("mut", GM.MUTANTS)
def test_mutants_are_rejected(mut):
    case = GM.case(GM.MUTANT_CASES[mut])
    for flip_v in (0, 1):
        assert TC.rejected(GM.check, case, GM.gbuffer_mesh_f32(case, None, flip_v, mut), None, flip_v, "gbm_mut", mut), (mut, case.name, flip_v)


# ---- irtobject.materials ---------------------------------------------------------------------------------------------------------------------------------------

def test_materials_accepts_what_the_docstring_says(tmp_path):
    from texir_code_amd import irtobject
    a, r = irtobject.materials("none", 3)
    assert a.dtype == r.dtype == np.float32 and a.shape == (3, 3) and r.shape == (3,) and (a == 0.5).all() and (r == 0.5).all()
    a, r = irtobject.materials(None, 0)
    assert a.shape == (0, 3) and r.shape == (0,)
    spec = [{"albedo": 0.25, "roughness": 0.01}, {"albedo": [0.1, 0.2, 3.0]}, {"roughness": 0.8}, {}]
    a, r = irtobject.materials(spec, 4)
    assert a.tolist() == np.array([[0.25] * 3, [0.1, 0.2, 3.0], [0.5] * 3, [0.5] * 3], np.float32).tolist()
    assert r.tolist() == np.array([0.01, 0.5, 0.8, 0.5], np.float32).tolist()
    bare, keyed = tmp_path / "bare.json", tmp_path / "keyed.json"
    bare.write_text(json.dumps(spec))
    keyed.write_text(json.dumps({"materials": spec}))
    for f in (bare, keyed):
        a2, r2 = irtobject.materials(str(f), 4)
        assert np.array_equal(a2, a) and np.array_equal(r2, r)


@pytest.mark.parametrize("spec,n", [([{"albedo": 0.5}], 2), ([], 1), ([{"albedo": -0.1}], 1), ([{"albedo": [0.1, float("nan"), 0.2]}], 1), ([{"albedo": float("inf")}], 1),
                                    ([{"albedo": [0.1, 0.2]}], 1), ([{"roughness": 0.009}], 1), ([{"roughness": 0.81}], 1), ([{"roughness": float("nan")}], 1),
                                    ([{"albedo": 0.5, "colour": 1}], 1), (["wood"], 1), ({"albedo": 0.5}, 1), ([{"albedo": "red"}], 1)])
def test_materials_refuses_and_names_the_key(spec, n):
    from texir_code_amd import irtobject
    with pytest.raises(ValueError, match="test.object_materials"):
        irtobject.materials(spec, n)


def test_materials_file_errors_name_the_key(tmp_path):
    from texir_code_amd import irtobject
    with pytest.raises(FileNotFoundError, match="test.object_materials"):
        irtobject.materials(str(tmp_path / "none.json"), 1)
    bad = tmp_path / "bad.json"
    bad.write_text("{")
    with pytest.raises(ValueError, match="test.object_materials"):
        irtobject.materials(str(bad), 1)


def test_parse_is_what_it_was():
    from texir_code_amd import irtobject
    with pytest.raises(ValueError, match="entry 0 must be \\{obj, pose\\}"):
        irtobject.parse([{"obj": "a.obj", "albedo": 0.5}])                           # a material is no key of an object entry


# ---- the evaluation model's conf keys ------------------------------------------------------------------------------------------------------------------------------

def test_draw_objects_settings():
    from texir_code_amd.tester import lit_model as LIT
    assert LIT.draw_objects_settings({}, None) == (False, None, 256)
    assert LIT.draw_objects_settings({"test.object_samples": 64, "test.object_materials": "no such file"}, None) == (False, None, 64)   # off: not read
    with pytest.raises(ValueError, match="test.draw_objects needs test.objects .*test.lights"):
        LIT.draw_objects_settings({"test.draw_objects": True}, None)
    for bad in ("true", 1, None):
        with pytest.raises(ValueError, match="test.draw_objects must be true or false"):
            LIT.draw_objects_settings({"test.draw_objects": bad}, None)
    for bad in (0, -1, 2.5, True, "many"):
        with pytest.raises(ValueError, match="test.object_samples"):
            LIT.draw_objects_settings({"test.object_samples": bad}, None)
    objects = {"occluders": [], "instances": [0, 0], "poses": np.zeros((2, 3, 4))}
    on, (a, r), n = LIT.draw_objects_settings({"test.draw_objects": True, "test.object_materials": [{"albedo": 0.2}, {"roughness": 0.3}]}, objects)
    assert on and n == 256 and a.shape == (2, 3) and abs(float(a[0, 0]) - 0.2) < 1e-7 and abs(float(r[1]) - 0.3) < 1e-7
    with pytest.raises(ValueError, match="test.object_materials has 1 entries for 2 objects"):
        LIT.draw_objects_settings({"test.draw_objects": True, "test.object_materials": [{}]}, objects)


# ---- the Python surface refuses what it can before it loads the library ---------------------------------------------------------------------------------------------------

def test_cast_gbuffer_refuses_bad_arguments_before_the_library(monkeypatch):
    import torch
    from texir_code_amd import _lib, gbuffer as GB

    def no_library():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "lib", no_library)
    mvp = torch.from_numpy(GC.cube_mvps(GC.GRAZE))
    with pytest.raises(ValueError, match="instances and poses need occluders"):
        GB.cast_gbuffer(None, mvp, 8, instances=[0], poses=np.zeros((1, 3, 4)))
    nine = [object()] * 9
    with pytest.raises(ValueError, match="at most 8 occluders and 8 instances"):
        GB.cast_gbuffer(None, mvp, 8, occluders=nine, instances=[0], poses=np.zeros((1, 3, 4)))
    with pytest.raises(ValueError, match="at most 8 occluders and 8 instances"):
        GB.cast_gbuffer(None, mvp, 8, occluders=[object()], instances=[0] * 9, poses=np.zeros((9, 3, 4)))
    with pytest.raises(ValueError, match="name no occluder"):
        GB.cast_gbuffer(None, mvp, 8, occluders=[object()], instances=[1], poses=np.zeros((1, 3, 4)))
    with pytest.raises(ValueError, match="name no occluder"):
        GB.cast_gbuffer(None, mvp, 8, occluders=[], instances=[0], poses=np.zeros((1, 3, 4)))
    for c in (0, 16385):
        with pytest.raises(ValueError, match="cube_res must be in 1..16384"):
            GB.cast_gbuffer(None, mvp, c, occluders=[], instances=[], poses=None)
    with pytest.raises(ValueError, match=r"mvp must be \[6,4,4\]"):
        GB.cast_gbuffer(None, mvp[:5], 8, occluders=[], instances=[], poses=None)
